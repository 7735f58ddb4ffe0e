"""What a burst's raw frames are in memory — normalised float32, uint16 sensor counts or packed uint8 rows — said once: the
record RawLayout (kind, width, levels; upload and normalisation) and what the entry points that take lists of frames share."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .utils_dng import _packing, infer_width, normalize_burst, normalize_packed, packed_row_bytes, to_uint16

FLOAT, COUNTS, PACKED = "float", "counts", "packed"


def host_counts(frame):
    """Is `frame` a host array of integer sensor counts?  Tensors and float data are taken as they are."""
    return not torch.is_tensor(frame) and np.issubdtype(np.asarray(frame).dtype, np.integer)


def upload_frame(frame, device, packed=False, counts_only=False):
    """One frame on `device` in its own form: packed uint8 rows stay uint8, any other integer array becomes uint16
    (ValueError outside its range), float data becomes float32 — or, with `counts_only`, is a TypeError."""
    floating = frame.dtype.is_floating_point if torch.is_tensor(frame) else not host_counts(frame)
    if floating and counts_only:
        raise TypeError("white balance: integer sensor counts expected: float frames are already white-balanced")
    if not torch.is_tensor(frame):
        a = np.asarray(frame)
        if floating:
            a = a.astype(np.float32, copy=False)
        elif not packed and a.dtype != np.uint16:
            a = to_uint16(a)
        frame = torch.as_tensor(np.ascontiguousarray(a))
    elif floating and frame.dtype != torch.float32:
        frame = frame.to(torch.float32)
    return frame.to(device, non_blocking=True)


class RawLayout(namedtuple("RawLayout", "kind packing width black_levels white_level", defaults=(None,) * 4)):
    """The raw frames of one burst: `kind` FLOAT (normalised, white-balanced; also whatever is not a host array of
    integers), COUNTS (uint16 sensor counts) or PACKED (uint8 rows [H, row_bytes] of 10/12/14-bit counts: `packing`, a
    name or id of utils_dng.PACKINGS, and `width` in pixels); counts of either form come with `black_levels` (R, G, B:
    a tuple of floats) and `white_level`.  Built by from_burst() or from_raw_norm()."""
    __slots__ = ()

    @classmethod
    def from_burst(cls, burst, ref):
        """From a burst mapping (process()) and its reference frame: integer host frames are counts, packed with the burst's
        `packing`; a missing `width` is the one whose rows have no padding (ValueError when `ref` has longer rows)."""
        if not host_counts(ref):
            return cls(FLOAT)
        levels = (tuple(float(v) for v in list(burst["black_levels"])[:3]), float(burst["white_level"]))
        if burst.get("packing", None) is None:
            return cls(COUNTS, None, None, *levels)
        packing = np.asarray(burst["packing"]).item()
        width = burst.get("width", None)
        width = infer_width(np.asarray(ref).shape[-1], packing) if width is None else int(np.asarray(width))
        if width is None:
            raise ValueError("packed burst: give 'width' (the rows are longer than their pixels' bytes)")
        return cls(PACKED, packing, width, *levels)

    @classmethod
    def from_raw_norm(cls, raw_norm, frame):
        """From config.hip.raw_norm and a frame tensor (BurstPipeline._ingest, graph.HostBurstRunner): only a 2-D uint8
        frame under a raw_norm with `packing` is packed; ValueError for a packing without a usable `width`."""
        if raw_norm is None or frame.dtype.is_floating_point:
            return cls(FLOAT)
        levels = (tuple(float(v) for v in list(raw_norm["black_levels"])[:3]), float(raw_norm["white_level"]))
        packing = raw_norm.get("packing", None)
        if packing is None or frame.dtype != torch.uint8 or frame.dim() != 2:
            return cls(COUNTS, None, None, *levels)
        if raw_norm.get("width", None) is None:
            raise ValueError("config.hip.raw_norm: 'packing' needs 'width', the pixels per row of the packed frames")
        width = int(raw_norm["width"])
        if width <= 0 or frame.shape[1] < packed_row_bytes(width, packing):
            raise ValueError(f"config.hip.raw_norm: 'width' {width} as {packing} needs rows of "
                             f"{packed_row_bytes(max(width, 1), packing)} bytes, the frames have {frame.shape[1]}")
        return cls(PACKED, packing, width, *levels)

    is_counts = property(lambda self: self.kind != FLOAT, doc="Sensor counts, uint16 or packed: to be normalised.")

    def upload(self, frame, device, counts_only=False):
        """upload_frame() of one of the burst's frames."""
        return upload_frame(frame, device, self.kind == PACKED, counts_only)

    def normalize(self, frames, white_balance, cfa_pattern, device=None):
        """Counts of this layout, [H, W] or [n, H, W], -> float32 GPU tensor (utils_dng.normalize_burst / normalize_packed)."""
        if self.kind == PACKED:
            return normalize_packed(frames, self.width, self.packing, self.black_levels, self.white_level, white_balance,
                                    cfa_pattern, device=device)
        return normalize_burst(frames, self.black_levels, self.white_level, white_balance, cfa_pattern, device=device)

    def raw_norm(self):
        """The config.hip.raw_norm that makes BurstPipeline normalise the burst's other frames like this."""
        out = {"black_levels": list(self.black_levels), "white_level": self.white_level}
        if self.kind == PACKED:
            out.update(packing=self.packing, width=self.width)
        return out


def frame_list(frames):
    """(list, device to work on: a frame's that is already on a GPU, else the current) of a frame, a stack or a list."""
    if torch.is_tensor(frames) or isinstance(frames, np.ndarray):
        frames = [frames] if frames.ndim == 2 else [frames[i] for i in range(frames.shape[0])]
    devs = [f.device for f in frames if torch.is_tensor(f) and f.is_cuda]
    return frames, devs[-1] if devs else torch.device("cuda", torch.cuda.current_device())


_WANTED = {(FLOAT,): "normalised float32 frames (got {})",
           (FLOAT, COUNTS, PACKED): "float32, uint16 or packed uint8 frames (got {})",
           (COUNTS, PACKED): "uint16 or packed uint8 sensor counts (got {}): normalised float frames are already "
                             "white-balanced"}


def check_device_frames(who, frames, kinds, packing=None, width=None):
    """(H, W, row_bytes, format code of hhsr_io.hip) of a non-empty list of device frames `who` was given: one 2-D shape,
    dtype, device and row stride, the elements of a row adjacent, and a dtype among `kinds` (a key of _WANTED) — float32
    (code 0), uint16 (-1) or, with `packing`, uint8 rows of `width` pixels (inferred when they hold no padding)."""
    if not frames:
        raise ValueError(f"{who}: no frame")
    f0 = frames[0]
    for t in frames:
        if not (torch.is_tensor(t) and t.is_cuda):
            raise RuntimeError(f"{who} expects tensors on the GPU (the HIP path has no CPU fallback)")
        if t.dim() != 2 or t.shape != f0.shape or t.dtype != f0.dtype or t.device != f0.device or t.stride() != f0.stride():
            raise ValueError(f"{who}: the frames need one 2-D shape, dtype, device and row stride")
    if f0.stride(1) != 1 and f0.shape[1] > 1:
        raise ValueError(f"{who}: the elements of a row must be adjacent in memory")
    H, row_bytes = f0.shape[0], f0.stride(0) * f0.element_size()
    if packing is not None and PACKED in kinds:
        if f0.dtype != torch.uint8:
            raise TypeError(f"{who}: packed frames are uint8 [H, row_bytes] (got {f0.dtype})")
        W = infer_width(f0.shape[1], packing) if width is None else int(width)
        if W is None:
            raise ValueError(f"{who}: give 'width' (the rows are longer than their pixels' bytes)")
        return H, W, row_bytes, _packing(packing)[0]
    kind, fmt = {torch.float32: (FLOAT, 0), torch.uint16: (COUNTS, -1), torch.int16: (COUNTS, -1)}.get(f0.dtype, (None, 0))
    if kind not in kinds:
        raise TypeError(f"{who}: " + _WANTED[tuple(kinds)].format(f0.dtype))
    return H, f0.shape[1], row_bytes, fmt


def summed_histogram(frames, shape, launch):
    """launch(chunk, hist) fills the int32 device tensor `hist` of `shape` for each chunk of up to MAX_BATCH of the device
    frames; the chunks' histograms, added (the int32 tensor holds the library's uint32 counts)."""
    dev, total = frames[0].device, None
    with torch.cuda.device(dev):
        for i in range(0, len(frames), _lib.MAX_BATCH):
            hist = torch.empty(shape, dtype=torch.int32, device=dev)
            launch(frames[i:i + _lib.MAX_BATCH], hist)
            total = hist if total is None else total.add_(hist)
    return total
