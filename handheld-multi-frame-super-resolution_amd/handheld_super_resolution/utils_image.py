"""Grey image (Alg. 3) and the decimating Gaussian (reference utils_image.py:58-112, 360-391)."""
import numpy as np
import torch

from . import _lib
from .raw_frames import COUNTS, FLOAT, PACKED, check_device_frames


class _GreyPlan:
    """Owner of one C-side hipFFT plan (H, W, device); destroyed with the object.  `batch`: spectra the plan holds =
    frames one launch per phase may carry (HHSR_GREY_BATCH)."""

    def __init__(self, H, W, batch=1):
        import ctypes
        import os

        _free_deferred_plans()
        h = ctypes.c_void_p()
        _lib.call("hhsr_grey_plan_create", H, W, int(os.environ.get("HHSR_GREY_PLAN", "4")) | (int(batch) << 8),
                  ctypes.byref(h))
        self.handle = h
        self.batch = int(batch)

    def __del__(self):
        # A plan owns hipMalloc'd buffers: destroying it calls hipFree, which is not permitted while the calling thread
        # captures a stream — and the garbage collector can run THIS finaliser in the middle of somebody's capture (an
        # engine dropped earlier whose graphs kept the plan alive: seen as "operation not permitted when stream is
        # capturing" + abort in tools/debug/emulate_ranks.py).  During a capture the handle is parked and freed later.
        try:
            if not self.handle:
                return
            h, self.handle = self.handle, None
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                _deferred_plans.append(h)
            else:
                _lib.load().hhsr_grey_plan_destroy(h)
        except Exception:
            pass


_deferred_plans = []  # handles of plans whose owner died during a stream capture


def _free_deferred_plans():
    """Destroy the parked plans (called where plans are created: never during a capture)."""
    if _deferred_plans and not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
        while _deferred_plans:
            try:
                _lib.load().hhsr_grey_plan_destroy(_deferred_plans.pop())
            except Exception:
                pass


_grey_plans = {}  # (H, W, device, stream) -> plan, least recently used first
_GREY_PLAN_CACHE = 16  # e.g. 4 streams x 2 image sizes (bench.py: full size, then the parity crop) x 2 devices


def _grey_plan(H, W, device, batch=1):
    """The plan of (size, device, stream); one that holds fewer spectra than `batch` is replaced by a larger one."""
    key = (H, W, device.index, torch.cuda.current_stream(device).cuda_stream)
    p = _grey_plans.pop(key, None)
    if p is not None and p.batch < batch:
        p = None
    if p is None:
        if torch.cuda.is_current_stream_capturing():
            # a plan allocates (twiddle tables, spectra): it has to exist before its stream is captured — graph.py's
            # runners do one eager call on the capture streams first
            raise RuntimeError(f"no FFT plan for {H}x{W} x{batch} on this stream yet: cannot create one during stream capture")
        while len(_grey_plans) >= _GREY_PLAN_CACHE:  # evict the least recently used plan only
            _grey_plans.pop(next(iter(_grey_plans)))
        with torch.cuda.device(device):
            p = _GreyPlan(H, W, batch)
    _grey_plans[key] = p  # most recently used last
    return p


def _grey_info_dict(rec):
    nm, nh = rec[9], rec[10]
    return {"fused": bool(rec[0]), "rows_per_workgroup": rec[1], "row_threads": rec[2], "cols_per_workgroup": rec[3],
            "static_rows": rec[4], "static_cols": rec[5], "lds_rows": rec[6], "lds_cols": rec[7], "kept_bins": rec[8],
            "radices_rows": list(rec[16:16 + nm]), "radices_cols": list(rec[32:32 + nh])}


def grey_plan_info(H, W, plan=None):
    """Which route the "FFT" grey image of an H x W frame takes: {"fused": the in-LDS kernels (else the library plans),
    rows / columns per workgroup, threads of the row kernels, ids of the compile-time plans (0: run-time passes), LDS bytes,
    kept x-bins, the radix schedules of the W/2-point ("radices_rows") and H-point ("radices_cols") transforms}.  Asked of
    the library's host side (hhsr_grey_plan_query, under the same HHSR_GREY_PLAN as a plan would be created): no GPU
    needed.  `plan`: report this live plan (of _grey_plan) instead."""
    import ctypes
    import os

    rec = (ctypes.c_int32 * _lib.GREY_INFO_LEN)()
    if plan is not None:
        _lib.call("hhsr_grey_plan_info", plan.handle, rec, _lib.GREY_INFO_LEN)
    else:
        _lib.call("hhsr_grey_plan_query", int(H), int(W), int(os.environ.get("HHSR_GREY_PLAN", "4")), rec,
                  _lib.GREY_INFO_LEN)
    return _grey_info_dict(list(rec))


def grey_radix_schedule(n, seqs=1, threads=512):
    """Radices of the passes that `seqs` simultaneous n-point transforms get in a workgroup of `threads` threads ([]: none)."""
    import ctypes

    rec = (ctypes.c_int32 * 17)()
    _lib.call("hhsr_grey_radix_schedule", int(n), int(seqs), int(threads), rec, 17)
    return list(rec[1:1 + rec[0]])


def plan_batch(n):
    """Spectra held by the plan that a launch of n frames uses.  A plan that serves more than one frame per launch always
    holds MAX_BATCH spectra — 24 MB each at 12 MP: the callers' chunk sizes vary, e.g. graph.host_chunks, and a plan cannot
    be replaced while its stream is captured; single frames (the reference frame, per-frame launches) need one."""
    return _lib.MAX_BATCH if n > 1 else 1


def compute_grey_images_batch(imgs, method="FFT"):
    """compute_grey_images() of a list of frames of one shape.  "FFT": ONE launch per transform phase for up to
    _lib.MAX_BATCH frames (hhsr_grey_lowpass_batch) instead of three per frame — the per-frame launches are
    latency-bound (row / column transforms that sit at barriers half of the time), a chunk of frames keeps one
    resident round of workgroups busy across the frames' row blocks.  Per frame bit-identical.  Returns a list of
    [H, W] views of one [n, H, W] tensor."""
    imgs = [_lib.f32c(i) for i in imgs]
    if method != "FFT":
        return [compute_grey_images(i, method) for i in imgs]
    H, W = imgs[0].shape
    dev = imgs[0].device
    outs = list(torch.empty((len(imgs), H, W), dtype=torch.float32, device=dev).unbind(0))
    _lib.call("hhsr_grey_lowpass_batch", _grey_plan(H, W, dev, plan_batch(len(imgs))).handle, _lib.ptr_array(imgs),
              _lib.ptr_array(outs), len(imgs), _lib.stream(dev))
    return outs


def compute_grey_images(img, method):
    """raw -> grey.  "FFT": ideal half-band low-pass (utils_image.py:82-100).  The reference runs a full
    complex FFT, zeroes the outer quarter bands of the shifted spectrum and keeps the real part; here the
    transforms are in-LDS HIP kernels (or rocFFT's real transform) inside libhhsr_hip.so and the zeroing is the
    equivalent Hermitian mask of the half spectrum (no fftshift copies), so the inverse returns the same real image.
    "decimating": 2x2 mean (utils_image.py:101-112) — only used inside the fused covariance kernel."""
    if method == "FFT":
        return compute_grey_images_batch([img])[0]
    img = _lib.f32c(img)
    H, W = img.shape
    if method == "FFT_torch":  # same maths through torch.fft (rocFFT behind torch), kept for cross-checking
        spec = torch.fft.rfft2(img)
        _lib.call("hhsr_lowpass_mask_r2c", _lib.ptr(spec), H, W, spec.stride(0), spec.stride(1), _lib.stream())
        return torch.fft.irfft2(spec, s=(H, W))
    if method == "FFT_c2c":  # the reference's literal formulation, kept for cross-checking the mask
        spec = torch.fft.fft2(img)
        _lib.call("hhsr_lowpass_mask_c2c", _lib.ptr(spec), H, W, spec.stride(0), spec.stride(1), _lib.stream())
        return torch.fft.ifft2(spec).real.contiguous()
    if method == "decimating":
        h, w = H // 2, W // 2
        v = img[: 2 * h, : 2 * w].double()
        return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]) / 4).float()
    raise NotImplementedError("Computation of gray level on GPU is only supported for FFT")


_taps_c = {}  # factor -> (ctypes float array, number of taps): built once, passed by pointer at every launch


def _taps_for_launch(factor):
    hit = _taps_c.get(factor)
    if hit is None:
        taps = gaussian_taps(factor)
        hit = _taps_c[factor] = (_lib.floats(taps), len(taps))
    return hit


def gaussian_taps(factor):
    """scipy.ndimage's 1-D Gaussian for sigma = factor/2, radius = int(2*factor + 0.5), as the reference
    requests it (utils_image.py:380), restated from its definition; float32 like the reference's tensor."""
    sigma = factor * 0.5
    radius = int(4 * factor * 0.5 + 0.5)
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return (phi / phi.sum()).astype(np.float32)


def cuda_downsample(th_img, kernel="gaussian", factor=2):
    """Valid separable Gaussian + decimation (utils_image.py:360-391) as ONE HIP kernel that writes a
    compact level (the reference returns a strided view of the filtered full-resolution image).
    Accepts [H, W] or [1, 1, H, W] like the reference's callers."""
    if factor == 1:
        return th_img
    if kernel != "gaussian":
        raise ValueError("please use gaussian kernel")
    out = cuda_downsample_batch([th_img.reshape(th_img.shape[-2:])], factor)[0]
    return out.reshape(*th_img.shape[:-2], *out.shape)


def cuda_downsample_batch(imgs, factor=2):
    """cuda_downsample() of a list of [H, W] levels of one shape in one launch (hhsr_gauss_decimate_batch); per frame
    bit-identical.  Returns a list of views of one [n, h2, w2] tensor."""
    if factor == 1:
        return list(imgs)
    imgs = [_lib.f32c(i) for i in imgs]
    H, W = imgs[0].shape
    taps, ntaps = _taps_for_launch(factor)
    r = (ntaps - 1) // 2
    h2, w2 = (H - 2 * r) // factor, (W - 2 * r) // factor
    if h2 < 1 or w2 < 1:
        raise ValueError(f"image of shape {(H, W)} is too small to be downsampled by {factor}")
    outs = list(torch.empty((len(imgs), h2, w2), dtype=torch.float32, device=imgs[0].device).unbind(0))
    _lib.call("hhsr_gauss_decimate_batch", _lib.ptr_array(imgs), len(imgs), H, W, W, _lib.ptr_array(outs), w2, factor,
              taps, ntaps, _lib.stream())
    return outs


# ---- after the path ------------------------------------------------------------------------------------
def apply_orientation(img, ori):
    """EXIF orientation 1..8 (utils_image.py:12-55).  NumPy arrays are handled like upstream; GPU tensors stay on the
    device ([H, W] planes through hhsr_orient_plane, images through flips / transposes of the same memory)."""
    ori = int(ori)
    if not torch.is_tensor(img):
        if ori == 2:
            img = np.flip(img, axis=1)
        elif ori == 3:
            img = np.rot90(img, k=2, axes=(0, 1))
        elif ori == 4:
            img = np.flip(img, axis=0)
        elif ori == 5:
            img = np.rot90(np.flip(img, axis=1), k=-3, axes=(0, 1))
        elif ori == 6:
            img = np.rot90(img, k=-1, axes=(0, 1))
        elif ori == 7:
            img = np.rot90(np.flip(img, axis=1), k=-1, axes=(0, 1))
        elif ori == 8:
            img = np.rot90(img, k=-3, axes=(0, 1))
        return img
    if ori == 1:
        return img
    if img.dim() == 2 and img.is_cuda:
        src = _lib.f32c(img)
        H, W = src.shape
        out = torch.empty((W, H) if ori >= 5 else (H, W), dtype=torch.float32, device=src.device)
        _lib.call("hhsr_orient_plane", _lib.ptr(src), _lib.ptr(out), H, W, ori, _lib.stream(src.device))
        return out
    t = {2: lambda a: a.flip(1), 3: lambda a: a.flip(0).flip(1), 4: lambda a: a.flip(0),
         5: lambda a: a.transpose(0, 1), 6: lambda a: a.transpose(0, 1).flip(1),
         7: lambda a: a.flip(0).flip(1).transpose(0, 1), 8: lambda a: a.transpose(0, 1).flip(0)}[ori]
    return t(img).contiguous()


# ---- reference selection: sharpness score of the candidate base frames (include/hhsr.h; no counterpart upstream) -------
def sharpness_workspace_bytes(H, W, n_frames):
    """Bytes of the partial sums of hhsr_frame_sharpness (the library's rule: hhsr_sharpness_workspace, no GPU needed)."""
    import ctypes

    out = ctypes.c_size_t()
    _lib.call("hhsr_sharpness_workspace", int(H), int(W), int(n_frames), ctypes.byref(out))
    return out.value


def frame_sharpness(frames, cfa_pattern=None, packing=None, width=None):
    """Sharpness scores of a list of device frames of one shape -> device float64 [n]: the float64 sum of the squared
    float32 differences of horizontally and vertically neighbouring values of the half-resolution green image
    (hhsr_frame_sharpness; include/hhsr.h states the score, tests/sharpness_ref.py is its NumPy form).  float32 [H, W]
    (any scale), uint16 [H, W] sensor counts, or with `packing` (a name of utils_dng.PACKINGS) uint8 [H, row_bytes] packed
    rows of `width` pixels (may be left out when the rows hold no padding) — read as they lie in memory, never normalised or
    copied: only the order of a burst's frames matters.  `cfa_pattern` None: a monochrome sensor (the mean of the four
    values of a quad).  Rows may be strided (raw_frames.check_device_frames).  The library is called in chunks of MAX_BATCH
    frames; a frame's score does not depend on the chunking."""
    frames = list(frames)
    H, W, row_bytes, fmt = check_device_frames("frame_sharpness", frames, (FLOAT, COUNTS, PACKED), packing, width)
    cfa = None if cfa_pattern is None else _lib.cfa_bytes(cfa_pattern)
    dev = frames[0].device
    scores = torch.empty(len(frames), dtype=torch.float64, device=dev)
    nbytes = sharpness_workspace_bytes(H, W, min(len(frames), _lib.MAX_BATCH))
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        for i in range(0, len(frames), _lib.MAX_BATCH):
            chunk = frames[i:i + _lib.MAX_BATCH]
            _lib.call("hhsr_frame_sharpness", _lib.ptr_array(chunk), len(chunk), H, W, row_bytes, fmt, cfa, _lib.ptr(work),
                      nbytes, _lib.ptr(scores[i:]), _lib.stream(dev))
    return scores


# ---- integer output (reference run_handheld.py:132-159, utils_dng.py:208-215) ------------------------------------------
OUTPUT_DTYPES = {"uint8": 8, "uint16": 16}


def _output_bits(dtype):
    name = dtype if isinstance(dtype, str) else str(np.dtype(dtype) if not isinstance(dtype, torch.dtype) else dtype)
    name = name.replace("torch.", "")
    if name not in OUTPUT_DTYPES:
        raise ValueError(f"integer output dtype {dtype!r}: one of {sorted(OUTPUT_DTYPES)}")
    return name, OUTPUT_DTYPES[name]


def encode_image(img, dtype, channels=None):
    """Device float32 [H, W, 3] or [H, W] -> device uint8 / uint16 of the same shape: rint(clip(nan_to_num(x), 0, 1) * M),
    half to even, M = 255 / 65535 (hhsr_encode_image; skimage's img_as_ubyte / the reference's 16-bit quantisation).
    `channels=1` of an [H, W, 3] image: channel 0 alone as [H, W] (`mode: grey`).  The kernel reads a compact image: a
    strided view goes through _lib.f32c, i.e. is copied first (not optimised).  process() never passes one — raw2rgb.postprocess
    stores the oriented image compactly, and with post-processing off apply_orientation has already made the rotated
    image contiguous, which is that same copy, one step earlier."""
    name, bits = _output_bits(dtype)
    if not (torch.is_tensor(img) and img.is_cuda):
        raise RuntimeError("encode_image expects a tensor on the GPU (the HIP path has no CPU fallback)")
    src = _lib.f32c(img)
    if src.dim() not in (2, 3) or (src.dim() == 3 and src.shape[2] not in (1, 3)):
        raise ValueError(f"encode_image expects [H, W] or [H, W, 3], got {tuple(src.shape)}")
    H, W = src.shape[:2]
    ch = 1 if src.dim() == 2 else src.shape[2]
    och = ch if channels is None else int(channels)
    if och not in (ch, 1):
        raise ValueError(f"channels={channels}: {ch} (all of them) or 1 (channel 0)")
    shape = (H, W) if (och == 1 and (src.dim() == 2 or channels is not None)) else (H, W, och)
    out = torch.empty(shape, dtype=getattr(torch, name), device=src.device)
    _lib.call("hhsr_encode_image", _lib.ptr(src), H, W, ch, och, _lib.ptr(out), bits, W * och * bits // 8,
              _lib.stream(src.device))
    return out


def robustness_mask(acc_r, n_comp, out_shape):
    """Oriented accumulated robustness, device float32 [ah, aw] -> device uint8 [mH, mW]: acc / n_comp, nearest-neighbour
    index (y * ah) // mH, quantised like encode_image (hhsr_encode_mask; the reference's `.rob.png`, one grey channel)."""
    if not (torch.is_tensor(acc_r) and acc_r.is_cuda):
        raise RuntimeError("robustness_mask expects a tensor on the GPU (the HIP path has no CPU fallback)")
    acc = _lib.f32c(acc_r)
    if acc.dim() != 2:
        raise ValueError(f"robustness_mask expects [ah, aw], got {tuple(acc.shape)}")
    mH, mW = (int(v) for v in out_shape)
    out = torch.empty((mH, mW), dtype=torch.uint8, device=acc.device)
    _lib.call("hhsr_encode_mask", _lib.ptr(acc), acc.shape[0], acc.shape[1], int(n_comp), _lib.ptr(out), mH, mW, mW,
              _lib.stream(acc.device))
    return out


def save_png(arr, path):
    """uint8 / uint16 ndarray [H, W] or [H, W, 3] -> PNG file, standard library only: filter type 0 on every row, 16-bit
    samples big-endian, zlib level 1 (a 48 MP image is written for its content, not its size)."""
    import struct
    import zlib

    a = np.asarray(arr)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.size == 0:
        raise ValueError(f"save_png expects uint8 / uint16 [H, W] or [H, W, 3], got {a.dtype} {a.shape}")
    H, W = a.shape[:2]
    rows = np.ascontiguousarray(a.astype(">u2") if a.dtype == np.uint16 else a).reshape(H, -1).view(np.uint8)
    raw = np.zeros((H, rows.shape[1] + 1), np.uint8)  # byte 0 of a row: its filter type
    raw[:, 1:] = rows

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", W, H, 8 * a.dtype.itemsize, 2 if a.ndim == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr))
        data = zlib.compress(raw.tobytes(), 1)
        for i in range(0, len(data), 1 << 30):  # (a chunk's length is a 31-bit field)
            f.write(chunk(b"IDAT", data[i:i + (1 << 30)]))
        f.write(chunk(b"IEND", b""))


# ---- JPEG output (include/hhsr.h "JPEG output"; the reference's imsave is cv2.imwrite on the host) ------------------------
JPEG_RESTART_MCUS = 64  # default restart interval, chosen by measurement (profiles/jpeg_encode.txt); the sweep for 4:2:0,
#                         whose MCUs are 16 x 16 pixels, keeps it (profiles/jpeg_subsampling.txt)


def jpeg_header(H, W, components, quality, restart_mcus):
    """The bytes in front of the scan (hhsr_jpeg_header: SOI .. SOS) as a uint8 ndarray."""
    import ctypes as C

    buf = (C.c_uint8 * 1024)()
    n = C.c_size_t(0)
    _lib.call("hhsr_jpeg_header", int(H), int(W), int(components), int(quality), int(restart_mcus), buf, 1024, C.byref(n))
    return np.frombuffer(buf, np.uint8, n.value).copy()


def jpeg_workspace(H, W, components, restart_mcus):
    """(bytes of the coefficients, bytes of the scratch, largest possible scan) of hhsr_jpeg_workspace."""
    import ctypes as C

    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    _lib.call("hhsr_jpeg_workspace", int(H), int(W), int(components), int(restart_mcus), C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


JPEG_SUBSAMPLINGS = {"444": 0, "420": 1}  # the `subsampling` argument of the hhsr_jpeg_*_ex entry points
JPEG_HUFFMAN = ("standard", "optimized")


def jpeg_option(name, value):
    """The canonical string of an encode_jpeg / config.output option: subsampling "444" | "420" (the integers too: YAML
    parses them as such), huffman "standard" | "optimized".  Anything else is a ValueError."""
    allowed = JPEG_SUBSAMPLINGS if name == "subsampling" else JPEG_HUFFMAN
    text = str(value) if isinstance(value, (str, int)) and not isinstance(value, bool) else None
    if text not in allowed:
        raise ValueError(f"{name}={value!r}: one of {', '.join(allowed)}")
    return text


def _jpeg_spec(spec, tables):
    """A table specification ([tables, 272] uint8, or None for K.3 - K.6) as the C ABI's argument."""
    import ctypes as C

    if spec is None:
        return None
    a = np.ascontiguousarray(spec, np.uint8)
    if a.shape != (tables, 272):
        raise ValueError(f"a Huffman specification of {tables} tables is uint8 [{tables}, 272], got {a.shape}")
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def jpeg_header_ex(H, W, components, quality, restart_mcus, subsampling=0, spec=None):
    """hhsr_jpeg_header_ex: jpeg_header for `subsampling` (0: 4:4:4, 1: 4:2:0) with the tables of `spec`."""
    import ctypes as C

    buf = (C.c_uint8 * 2048)()
    n = C.c_size_t(0)
    _lib.call("hhsr_jpeg_header_ex", int(H), int(W), int(components), int(quality), int(restart_mcus), int(subsampling),
              _jpeg_spec(spec, 2 if int(components) == 1 else 4), buf, 2048, C.byref(n))
    return np.frombuffer(buf, np.uint8, n.value).copy()


def jpeg_workspace_ex(H, W, components, restart_mcus, subsampling=0):
    """(bytes of the coefficients, bytes of the scratch, largest possible scan) of hhsr_jpeg_workspace_ex."""
    import ctypes as C

    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    _lib.call("hhsr_jpeg_workspace_ex", int(H), int(W), int(components), int(restart_mcus), int(subsampling), C.byref(a),
              C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def jpeg_huffman(counts):
    """hhsr_jpeg_huffman: symbol counts [2 or 4, 256] (host) -> the optimal table specification, uint8 [2 or 4, 272]."""
    import ctypes as C

    c = np.ascontiguousarray(counts, np.uint64)
    if c.ndim != 2 or c.shape[1] != 256:
        raise ValueError(f"jpeg_huffman expects counts [2 or 4, 256], got {c.shape}")
    spec = np.zeros((c.shape[0], 272), np.uint8)
    _lib.call("hhsr_jpeg_huffman", c.ctypes.data_as(C.POINTER(C.c_uint64)), int(c.shape[0]),
              spec.ctypes.data_as(C.POINTER(C.c_uint8)))
    return spec


def encode_jpeg(img, quality=90, restart_mcus=None, channels=None, capacity=None, subsampling="444", huffman="standard"):
    """Device float32 [H, W, 3] or [H, W] -> the complete baseline JPEG file as a 1-D uint8 ndarray (hhsr_jpeg_dct,
    hhsr_jpeg_entropy): the samples of encode_image(img, "uint8"), 4:4:4, the standard tables at `quality` (IJG scaling),
    restart intervals of `restart_mcus` MCUs (default JPEG_RESTART_MCUS).  `channels=1` of an [H, W, 3] image: channel 0
    alone as a grey file (`mode: grey`).  Only the length word and the file's bytes cross the host link: the scan is coded
    into `capacity` device bytes (default 2 H W C; noise at quality 100 was measured at 1.4 bytes per sample), the length
    word is read, exactly that many bytes are copied; a scan that did not fit is coded once more into a buffer of the
    reported length.

    `subsampling="420"` (three components only): Cb and Cr at half resolution in both directions, MCUs of 16 x 16 pixels,
    which `restart_mcus` then counts.  `huffman="optimized"`: the tables are made for this image — hhsr_jpeg_histogram
    counts the scan's symbols on the device, the 8 KB of counts are copied to the host, hhsr_jpeg_huffman builds the
    tables, they go into the header and back to the coder as code words.  That is ONE MORE SYNCHRONISATION than the
    standard tables need (the copy of the counts, before the scan can be coded).  Either option goes through the
    hhsr_jpeg_*_ex entry points; with both at their defaults the calls are exactly those of the four original ones."""
    if not (torch.is_tensor(img) and img.is_cuda):
        raise RuntimeError("encode_jpeg expects a tensor on the GPU (the HIP path has no CPU fallback)")
    src = _lib.f32c(img)
    if src.dim() not in (2, 3) or (src.dim() == 3 and src.shape[2] not in (1, 3)):
        raise ValueError(f"encode_jpeg expects [H, W] or [H, W, 3], got {tuple(src.shape)}")
    H, W = src.shape[:2]
    ch = 1 if src.dim() == 2 else src.shape[2]
    och = ch if channels is None else int(channels)
    if och not in (ch, 1):
        raise ValueError(f"channels={channels}: {ch} (all of them) or 1 (channel 0)")
    quality = int(quality)
    ri = JPEG_RESTART_MCUS if restart_mcus is None else int(restart_mcus)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality={quality}: 1 .. 100")
    if not 1 <= ri <= 65535:
        raise ValueError(f"restart_mcus={ri}: 1 .. 65535")
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"a JPEG holds at most 65535 x 65535 pixels, got {H} x {W}")
    sub = JPEG_SUBSAMPLINGS[jpeg_option("subsampling", subsampling)]
    optimized = jpeg_option("huffman", huffman) == "optimized"
    if sub and och != 3:
        raise ValueError("subsampling=420 needs three components")
    ex = bool(sub or optimized)
    dev, stream = src.device, _lib.stream(src.device)
    coef_bytes, scratch_bytes, _ = jpeg_workspace_ex(H, W, och, ri, sub) if ex else jpeg_workspace(H, W, och, ri)
    coef = torch.empty(coef_bytes // 2, dtype=torch.int16, device=dev)
    scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
    length = torch.empty(1, dtype=torch.int64, device=dev)
    spec = None
    if not ex:
        head = jpeg_header(H, W, och, quality, ri)
        _lib.call("hhsr_jpeg_dct", _lib.ptr(src), H, W, ch, och, quality, _lib.ptr(coef), coef_bytes, stream)
    else:
        _lib.call("hhsr_jpeg_dct_ex", _lib.ptr(src), H, W, ch, och, quality, sub, _lib.ptr(coef), coef_bytes, stream)
        if optimized:
            counts = torch.empty((4, 256), dtype=torch.int64, device=dev)
            _lib.call("hhsr_jpeg_histogram", _lib.ptr(coef), H, W, och, sub, ri, _lib.ptr(counts), _lib.ptr(scratch),
                      scratch.numel() * 8, stream)
            tables = 2 if och == 1 else 4
            spec = jpeg_huffman(counts.cpu().numpy().view(np.uint64)[:tables])  # (synchronises: the 8 KB of counts)
        head = jpeg_header_ex(H, W, och, quality, ri, sub, spec)
    cap = 2 * H * W * och if capacity is None else int(capacity)
    for _ in range(2):  # at most one retry, with the length the first pass reported
        scan = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        if not ex:
            _lib.call("hhsr_jpeg_entropy", _lib.ptr(coef), H, W, och, ri, _lib.ptr(scratch), scratch.numel() * 8,
                      _lib.ptr(scan), cap, _lib.ptr(length), stream)
        else:
            _lib.call("hhsr_jpeg_entropy_ex", _lib.ptr(coef), H, W, och, ri, sub, _jpeg_spec(spec, 2 if och == 1 else 4),
                      _lib.ptr(scratch), scratch.numel() * 8, _lib.ptr(scan), cap, _lib.ptr(length), stream)
        n = int(length.item())  # (synchronises: the one 8-byte read)
        if n < 0:  # UINT64_MAX (cannot happen with tables counted at the same interval)
            raise RuntimeError("encode_jpeg: the Huffman tables lack a symbol the scan needs")
        if n <= cap:
            break
        cap = n
    else:
        raise RuntimeError(f"encode_jpeg: the scan needs {n} bytes after a retry with the reported length")
    out = np.empty(head.size + n + 2, np.uint8)
    out[:head.size] = head
    out[head.size:head.size + n] = scan[:n].cpu().numpy()
    out[-2:] = (0xFF, 0xD9)  # EOI
    return out


def save_jpeg(file_bytes, path):
    """The array encode_jpeg (or process() with output.format = jpeg) returned -> a file."""
    a = np.asarray(file_bytes)
    if a.dtype != np.uint8 or a.ndim != 1 or a.size < 4 or a[0] != 0xFF or a[1] != 0xD8:
        raise ValueError("save_jpeg expects the 1-D uint8 array of encode_jpeg")
    with open(path, "wb") as f:
        f.write(a.tobytes())


# ---- PNG output (include/hhsr.h "PNG output"; the reference's imsave writes its PNG on the host) ----------------------------------
PNG_INTERVAL_BYTES = 65536  # default interval of the deflate coder, chosen by measurement (profiles/png_encode.txt: the fastest
#                            of 4 KiB .. 256 KiB whose file is within 1 % of the largest interval's, at 8 and at 16 bits)
PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}  # the `filter` argument of hhsr_png_filter


def png_option(name, value):
    """The canonical value of an encode_png / config.output option: filter -> one of PNG_FILTERS' names, interval_bytes ->
    an int in 1 .. 2^20 (None: PNG_INTERVAL_BYTES).  Anything else is a ValueError."""
    if name == "filter":
        if not isinstance(value, str) or value not in PNG_FILTERS:
            raise ValueError(f"filter={value!r}: one of {', '.join(PNG_FILTERS)}")
        return value
    if name == "interval_bytes":
        if value is None:
            return PNG_INTERVAL_BYTES
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= 1 << 20:
            raise ValueError(f"interval_bytes={value!r}: an integer in 1 .. {1 << 20}")
        return int(value)
    raise ValueError(f"png_option: no option {name!r}")


def png_workspace(H, W, components, bits, interval_bytes):
    """(bytes of the filtered stream, bytes of the scratch, largest possible deflate stream) of hhsr_png_workspace."""
    import ctypes as C

    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    _lib.call("hhsr_png_workspace", int(H), int(W), int(components), int(bits), int(interval_bytes), C.byref(a), C.byref(b),
              C.byref(c))
    return a.value, b.value, c.value


def png_huffman(counts):
    """hhsr_png_huffman: counts [257] (host; [256]: the number of intervals) -> spec, uint8 [_lib.PNG_SPEC_BYTES]: the
    optimal code lengths under the 15-bit limit and the header of a dynamic-Huffman block."""
    import ctypes as C

    c = np.ascontiguousarray(counts, np.uint64)
    if c.shape != (257,):
        raise ValueError(f"png_huffman expects counts [257], got {c.shape}")
    spec = np.zeros(_lib.PNG_SPEC_BYTES, np.uint8)
    _lib.call("hhsr_png_huffman", c.ctypes.data_as(C.POINTER(C.c_uint64)), spec.ctypes.data_as(C.POINTER(C.c_uint8)))
    return spec


def png_file_head(H, W, components, bits, deflate_len):
    """hhsr_png_file_head: signature, IHDR, the IDAT chunk's length and type, 78 01 — as a uint8 ndarray."""
    import ctypes as C

    buf, n = (C.c_uint8 * 64)(), C.c_size_t(0)
    _lib.call("hhsr_png_file_head", int(H), int(W), int(components), int(bits), int(deflate_len), buf, 64, C.byref(n))
    return np.frombuffer(buf, np.uint8, n.value).copy()


def png_file_tail(deflate_crc, deflate_len, adler):
    """hhsr_png_file_tail: the Adler-32, the IDAT chunk's CRC, IEND — as a uint8 ndarray."""
    import ctypes as C

    buf, n = (C.c_uint8 * 32)(), C.c_size_t(0)
    _lib.call("hhsr_png_file_tail", int(deflate_crc), int(deflate_len), int(adler), buf, 32, C.byref(n))
    return np.frombuffer(buf, np.uint8, n.value).copy()


def png_crc_combine(crc_a, crc_b, len_b):
    """hhsr_png_crc_combine: crc32(A || B) from crc32(A), crc32(B) and len(B)."""
    import ctypes as C

    out = C.c_uint32(0)
    _lib.call("hhsr_png_crc_combine", int(crc_a), int(crc_b), int(len_b), C.byref(out))
    return out.value


def encode_png(img, bits=8, channels=None, filter="adaptive", interval_bytes=None, capacity=None):  # noqa: A002 (PNG's word)
    """Device float32 [H, W, 3] or [H, W] -> the complete PNG file as a 1-D uint8 ndarray, filtered and deflate-coded on
    the device (hhsr_png_filter, hhsr_png_deflate): the samples of encode_image(img, uint8 / uint16), colour type 2 or 0,
    `filter` on every row ("adaptive": libpng's per-row choice), Huffman-only deflate with one code for the image and one
    block per `interval_bytes` of the filtered stream (default PNG_INTERVAL_BYTES).  `channels=1` of an [H, W, 3] image:
    channel 0 alone as a grey file (`mode: grey`).  Two synchronisations, as encode_jpeg(huffman="optimized"): the 2 KB of
    byte counts are copied, hhsr_png_huffman builds the code on the host, the stream is coded into `capacity` device bytes
    (default: the bound of hhsr_png_workspace), the three result words — length, CRC-32 of the deflate stream, Adler-32 of
    the filtered stream, all made on the device — are read, and exactly the stream's bytes are copied; a stream that did
    not fit is coded once more into a buffer of the reported length."""
    if not (torch.is_tensor(img) and img.is_cuda):
        raise RuntimeError("encode_png expects a tensor on the GPU (the HIP path has no CPU fallback)")
    src = _lib.f32c(img)
    if src.dim() not in (2, 3) or (src.dim() == 3 and src.shape[2] not in (1, 3)):
        raise ValueError(f"encode_png expects [H, W] or [H, W, 3], got {tuple(src.shape)}")
    H, W = src.shape[:2]
    ch = 1 if src.dim() == 2 else src.shape[2]
    och = ch if channels is None else int(channels)
    if och not in (ch, 1):
        raise ValueError(f"channels={channels}: {ch} (all of them) or 1 (channel 0)")
    if bits not in (8, 16):
        raise ValueError(f"bits={bits!r}: 8 or 16")
    ftype = PNG_FILTERS[png_option("filter", filter)]
    interval = png_option("interval_bytes", interval_bytes)
    if H < 1 or W < 1 or H * (1 + W * och * bits // 8) > (1 << 31) - 1:
        raise ValueError(f"encode_png: {H} x {W} does not fit one IDAT chunk (2^31 - 1 bytes)")
    dev, stream = src.device, _lib.stream(src.device)
    n, scratch_bytes, bound = png_workspace(H, W, och, bits, interval)
    filtered = torch.empty(n, dtype=torch.uint8, device=dev)
    scratch = torch.empty((scratch_bytes + 7) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty(256, dtype=torch.int64, device=dev)
    result = torch.empty(3, dtype=torch.int64, device=dev)
    _lib.call("hhsr_png_filter", _lib.ptr(src), H, W, ch, och, bits, ftype, _lib.ptr(filtered), n, _lib.ptr(counts),
              _lib.ptr(scratch), scratch.numel() * 8, stream)
    c257 = np.empty(257, np.uint64)
    c257[:256] = counts.cpu().numpy().view(np.uint64)  # (synchronises: the 2 KB of counts)
    c257[256] = -(-n // interval)
    spec = png_huffman(c257)
    import ctypes as C

    spec_p = spec.ctypes.data_as(C.POINTER(C.c_uint8))
    cap = bound if capacity is None else int(capacity)
    for _ in range(2):  # at most one retry, with the length the first pass reported
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        _lib.call("hhsr_png_deflate", _lib.ptr(filtered), n, interval, spec_p, _lib.ptr(scratch), scratch.numel() * 8,
                  _lib.ptr(out), cap, _lib.ptr(result), stream)
        length, crc, adler = (int(v) for v in result.cpu().numpy().view(np.uint64))  # (synchronises: the 24 bytes)
        if length == (1 << 64) - 1:  # (cannot happen with a code built from this stream's counts)
            raise RuntimeError("encode_png: the code lacks a byte value the stream holds")
        if length <= cap:
            break
        cap = length
    else:
        raise RuntimeError(f"encode_png: the stream needs {length} bytes after a retry with the reported length")
    head, tail = png_file_head(H, W, och, bits, length), png_file_tail(crc, length, adler)
    data = np.empty(head.size + length + tail.size, np.uint8)
    data[:head.size] = head
    torch.from_numpy(data)[head.size:head.size + length].copy_(out[:length])  # (device -> its place in the file: one host copy)
    data[head.size + length:] = tail
    return data


def save_png_bytes(file_bytes, path):
    """The array encode_png (or process() with output.format = png) returned -> a file."""
    a = np.asarray(file_bytes)
    if a.dtype != np.uint8 or a.ndim != 1 or a.size < 8 or a[:8].tobytes() != b"\x89PNG\r\n\x1a\n":
        raise ValueError("save_png_bytes expects the 1-D uint8 array of encode_png")
    with open(path, "wb") as f:
        f.write(a.tobytes())


def _frame_count_denoise(image, r_acc, config, kind, strength, scale, half_index, mode=None):
    # `mode: grey` (monochrome sensors): the reference indexes the accumulated robustness with int(round(y / scale))
    # (utils_image.py:203-204, 260-261) instead of the Bayer branch's half-resolution index.  Upstream reads `mode` (and
    # `scale`) from the denoiser's own sub-block, which process() never fills: here process() passes both.
    mode = str(config.get("mode", "bayer") if mode is None else mode)
    if mode == "grey":
        half_index = 2
    scale = config.get("scale", scale)
    if scale is None:
        raise ValueError("the frame-count denoisers need the scale (config.scale or the scale argument)")
    img = _lib.f32c(image)
    acc = _lib.f32c(r_acc, img.device)
    H, W, C = img.shape
    assert C == 3
    out = torch.empty_like(img)
    _lib.call("hhsr_frame_count_denoise", _lib.ptr(img), _lib.ptr(out), H, W, _lib.ptr(acc), acc.shape[0], acc.shape[1],
              float(scale), kind, float(strength), float(config.max_frame_count), int(half_index),
              _lib.stream(img.device))
    return out


def frame_count_denoising_median(image, r_acc, config, scale=None, half_index=True, mode=None):
    """Median filter whose radius grows where few frames were merged (utils_image.py:236-286).  `config`: the
    accumulated_robustness_denoiser.median block (radius_max <= 7, max_frame_count); the reference reads `scale` and
    `mode` from the same block although process() never puts them there — pass `scale`.  `half_index`: keep the
    reference's index into the accumulated robustness (it addresses the [H, W] map at half resolution)."""
    return _frame_count_denoise(image, r_acc, config, 0, config.radius_max, scale, half_index, mode)


def frame_count_denoising_gauss(image, r_acc, config, scale=None, half_index=True, mode=None):
    """Gaussian blur whose sigma grows where few frames were merged (utils_image.py:174-234).  Upstream this kernel does
    not compile (range() of the float 3 sigma); the build's window is |i|, |j| <= ceil(3 sigma)."""
    return _frame_count_denoise(image, r_acc, config, 1, config.sigma_max, scale, half_index, mode)
