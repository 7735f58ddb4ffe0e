"""Shared by the lossless-JPEG tests: streams of tests/ljpeg_ref.py laid out as segments of an image, the arguments of
hhsr_ljpeg_decode / hhsr_ljpeg_decode_host built from them through the library's own parser, and the two calls with the
output inside guard bands."""
import ctypes
from collections import namedtuple

import numpy as np

import ljpeg_ref

GUARD = 0xA5C3
Plan = namedtuple("Plan", "blob segments tables workspace_elems n_frames H W")


def plan_from_streams(items, n_frames, H, W, lead=0, dedup=True):
    """items: (stream bytes, frame, x0, y0, seg_w, seg_h) per segment -> Plan.  The entropy-coded bytes start `lead` bytes
    into the blob and follow each other without padding; the blob ends with its last segment's last byte when that is on
    a multiple of 4 (else zero padding)."""
    from handheld_super_resolution import _lib
    from handheld_super_resolution.dng import parse_ljpeg

    chunks, descs, keys, at = [b"\0" * lead], [], {}, lead
    for stream, frame, x0, y0, seg_w, seg_h in items:
        lj = parse_ljpeg(stream)
        d = _lib.LjpegSegment(offset=at, length=lj.data_length, X=lj.X, Y=lj.Y, Nf=lj.Nf, P=lj.P, predictor=lj.predictor,
                              frame=frame, x0=x0, y0=y0, seg_w=seg_w, seg_h=seg_h)
        for c in range(lj.Nf):
            key = (bytes(lj.bits[lj.table[c]]), bytes(lj.values[lj.table[c]]))
            d.table[c] = keys.setdefault(key if dedup else (key, len(descs), c), len(keys))
        chunks.append(stream[lj.data_offset:lj.data_offset + lj.data_length])
        at += lj.data_length
        descs.append(d)
    blob = np.zeros(-(-at // 4) * 4, np.uint8)
    blob[:at] = np.frombuffer(b"".join(chunks), np.uint8)
    segs = (_lib.LjpegSegment * len(descs))(*descs)
    klist = [k if dedup else k[0] for k in keys]
    tables = (_lib.LjpegTable * len(klist))()
    _lib.call("hhsr_ljpeg_tables", b"".join(k[0] for k in klist), b"".join(k[1] for k in klist), len(klist),
              ctypes.addressof(tables))
    ws = ctypes.c_size_t()
    _lib.call("hhsr_ljpeg_workspace", ctypes.addressof(segs), len(descs), ctypes.byref(ws))
    return Plan(blob, segs, tables, ws.value // 2, n_frames, H, W)


def decode_host(plan, row_elems=None, band=32):
    """hhsr_ljpeg_decode_host into a guarded, pitched buffer -> (counts [n, H, W], statuses, guards intact?)."""
    from handheld_super_resolution import _lib

    n, H, W = plan.n_frames, plan.H, plan.W
    row = W if row_elems is None else row_elems
    buf = np.full(band + n * H * row + band, GUARD, np.uint16)
    work = np.full(band + max(1, plan.workspace_elems) + band, GUARD, np.uint16)
    status = np.full(len(plan.segments), -7, np.int32)
    _lib.call("hhsr_ljpeg_decode_host", plan.blob.ctypes.data, plan.blob.size, ctypes.addressof(plan.segments),
              len(plan.segments), ctypes.addressof(plan.tables), len(plan.tables), work[band:].ctypes.data,
              plan.workspace_elems * 2, buf[band:].ctypes.data, n, H, W, row, H * row, status.ctypes.data)
    img = buf[band:band + n * H * row].reshape(n, H, row)
    intact = bool((buf[:band] == GUARD).all() and (buf[-band:] == GUARD).all() and (img[:, :, W:] == GUARD).all()
                  and (work[:band] == GUARD).all() and (work[-band:] == GUARD).all())
    return img[:, :, :W].copy(), status, intact


def decode_gpu(plan, row_elems=None, band=32):
    """hhsr_ljpeg_decode the same way on the current device."""
    import torch

    from handheld_super_resolution import _lib

    n, H, W = plan.n_frames, plan.H, plan.W
    row = W if row_elems is None else row_elems
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.full((band + n * H * row + band,), GUARD - 65536, dtype=torch.int16, device=dev)
    work = torch.full((band + max(1, plan.workspace_elems) + band,), GUARD - 65536, dtype=torch.int16, device=dev)
    status = torch.full((len(plan.segments),), -7, dtype=torch.int32, device=dev)
    blob = torch.as_tensor(plan.blob).to(dev)
    segs = torch.as_tensor(np.frombuffer(plan.segments, np.uint8).copy()).to(dev)
    tabs = torch.as_tensor(np.frombuffer(plan.tables, np.uint8).copy()).to(dev)
    _lib.call("hhsr_ljpeg_decode", _lib.ptr(blob), blob.numel(), _lib.ptr(segs), len(plan.segments), _lib.ptr(tabs),
              len(plan.tables), ctypes.c_void_p(work.data_ptr() + 2 * band), plan.workspace_elems * 2,
              ctypes.c_void_p(buf.data_ptr() + 2 * band), n, H, W, row, H * row, _lib.ptr(status), _lib.stream())
    torch.cuda.synchronize()
    b = buf.cpu().numpy().view(np.uint16)
    w = work.cpu().numpy().view(np.uint16)
    img = b[band:band + n * H * row].reshape(n, H, row)
    intact = bool((b[:band] == GUARD).all() and (b[-band:] == GUARD).all() and (img[:, :, W:] == GUARD).all()
                  and (w[:band] == GUARD).all() and (w[-band:] == GUARD).all())
    return img[:, :, :W].copy(), status.cpu().numpy(), intact


def segment_streams(counts, P, layout, size, Nf=1, X=None, predictor=1, tables="k2", frame_of=None):
    """counts [n, H, W] cut into tiles (`layout` "tiles", `size` (tw, th): edge tiles padded by repeating the last column /
    row, as DNG writers do) or strips of `size` rows -> the items of plan_from_streams.  Each segment's rectangle is coded
    FLAT as lines of X Nf samples (default X = seg_w / Nf).  predictor / tables may be callables of the segment's index."""
    n, H, W = counts.shape
    items, k = [], 0
    for f in range(n):
        if layout == "tiles":
            tw, th = size
            rects = [(x0, y0, tw, th) for y0 in range(0, H, th) for x0 in range(0, W, tw)]
        else:
            rects = [(0, y0, W, min(size, H - y0)) for y0 in range(0, H, size)]
        for x0, y0, w, h in rects:
            rect = counts[f, y0:y0 + h, x0:x0 + w]
            rect = np.pad(rect, ((0, h - rect.shape[0]), (0, w - rect.shape[1])), mode="edge")
            x = (w // Nf) if X is None else X
            s = ljpeg_ref.to_stream_geometry(rect, Nf, x)
            pr = predictor(k) if callable(predictor) else predictor
            tb = tables(k) if callable(tables) else tables
            items.append((ljpeg_ref.encode(s, P, pr, tables=tb), f, x0, y0, w, h))
            k += 1
    return items
