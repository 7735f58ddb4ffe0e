"""Coarse-to-fine alignment driver (reference alignment.py).

Flow convention: alignments[ty, tx] = (dx, dy), moving(p + flow) ~= ref(p).  Pyramids are COARSE FIRST
like the reference's lists."""
import torch
import torch.nn.functional as F

from . import _lib
from .config import hip_opt
from .ICA import init_ica, align_lvl_ica
from .block_matching import align_lvl_block_matching_L2, align_lvl_block_matching_L1
from .utils_image import cuda_downsample_batch


def build_gaussian_pyramid(image, factors=[1, 2, 4, 4], kernel="gaussian"):
    """alignment.py:74-82: compact contiguous levels, coarse first."""
    if kernel != "gaussian":
        raise ValueError("please use gaussian kernel")
    return build_gaussian_pyramids([image.reshape(image.shape[-2:])], factors)[0]


def build_gaussian_pyramids(images, factors=[1, 2, 4, 4]):
    """build_gaussian_pyramid() of several frames of one shape, one launch per level (coarse first per frame)."""
    levels = [cuda_downsample_batch(images, factors[0])]
    for factor in factors[1:]:
        levels.append(cuda_downsample_batch(levels[-1], factor))
    return [[lvl[i] for lvl in levels[::-1]] for i in range(len(images))]


def init_alignment(ref_img, config):
    """Reference-side precompute (alignment.py:20-72): circular pad to a multiple of the tile size,
    pyramid, per-level gradients + Hessian.

    Returns the reference's 6-tuple (pyramid, tiled_pyr, tiled_fft, gradx, grady, hessian), coarse first.
    The tiled / FFT'd copies of the reference tiles exist upstream only to feed the FFT correlation; the
    LDS block-matching kernel reads the level directly, so those two lists hold None."""
    ref_img = _lib.f32c(ref_img)
    h, w = ref_img.shape
    bm = config.block_matching.tuning
    Ts, tss, factors = bm.tile_size, bm.tile_sizes, bm.factors
    pb = (Ts - h % Ts) * (h % Ts != 0)
    pr = (Ts - w % Ts) * (w % Ts != 0)
    if pb or pr:
        padded = torch.empty((h + pb, w + pr), dtype=torch.float32, device=ref_img.device)
        _lib.call("hhsr_pad_circular", _lib.ptr(ref_img), h, w, w, _lib.ptr(padded), h + pb, w + pr, w + pr,
                  _lib.stream())
    else:
        padded = ref_img
    pyramid = build_gaussian_pyramid(padded, factors)
    gxs, gys, hs = [], [], []
    for i, lvl in enumerate(pyramid):
        ts = tss[len(factors) - i - 1]
        if lvl.shape[0] // ts < 1 or lvl.shape[1] // ts < 1:
            raise ValueError(f"pyramid level of shape {tuple(lvl.shape)} cannot be divided into tiles of size {ts}")
        gx, gy, hess = init_ica(lvl, ts, config)
        gxs.append(gx)
        gys.append(gy)
        hs.append(hess)
    none = [None] * len(pyramid)
    return pyramid, list(none), list(none), gxs, gys, hs


def upscale_lvl(alignments, npatchs, l, config):
    """Re-tile and scale the flow for the next finer level (alignment.py:150-172)."""
    bm = config.block_matching.tuning
    new_ts, prev_ts = bm.tile_sizes[l], bm.tile_sizes[l + 1]
    up = bm.factors[l + 1]
    rep = up // (new_ts // prev_ts)
    mode = bm.flow_upscale_mode
    sny, snx, _ = alignments.shape
    if mode == "nearest":
        out = torch.empty((npatchs[0], npatchs[1], 2), dtype=torch.float32, device=alignments.device)
        _lib.call("hhsr_flow_upscale_nearest", _lib.ptr(alignments), sny, snx, _lib.ptr(out), npatchs[0], npatchs[1],
                  rep, float(up), _lib.stream())
        return out
    # bilinear / bicubic: the reference itself delegates to F.interpolate on this <= 188x250x2 field
    ups = F.interpolate(alignments.permute(2, 0, 1)[None], scale_factor=rep, mode=mode)[0].permute(1, 2, 0)
    ups = ups * up
    py, px = npatchs[0] - ups.shape[0], npatchs[1] - ups.shape[1]
    if py > 0 or px > 0:
        ups = F.pad(ups, (0, 0, 0, max(px, 0), 0, max(py, 0)), mode="constant", value=0)
    return ups[: npatchs[0], : npatchs[1]].contiguous()


def _fused_level(l, config):
    """(metric code, ts, r) when level l runs on the fused block-matching + ICA kernel, else None."""
    bm = config.block_matching.tuning
    ts, r = bm.tile_sizes[l], bm.search_radii[l]
    fused = bool(hip_opt(config, "fused_align"))
    code = {"L2": 0, "L1": 1, "L1_ref_effective": 2}.get(bm.metrics[l])
    if fused and code is not None and ts in (8, 16, 32) and r in (1, 2, 4) and not (code != 0 and ts == 8):
        return code, ts, r
    return None


def _align_level_fused(fl, ref_lvl, ref_hessian_lvl, movs, flows, coarse, config):
    """ONE launch of the fused block-matching + ICA kernel for a list of frames (hhsr_align_level_batch).  `coarse`: where
    the incoming flows come from instead of `flows` — None (in place), "zero" or (coarser flows, rep, mult) for the
    nearest-neighbour upscaling of upscale_lvl() fused into the launch; `flows` then only receive the result."""
    code, ts, r = fl
    ny, nx, _ = flows[0].shape
    mh, mw = movs[0].shape
    rh, rw = ref_lvl.shape
    assert ref_lvl.is_contiguous() and all(t.is_contiguous() for t in (*movs, *flows))
    if coarse is None:
        cptr, cny, cnx, rep, mult = None, 0, 0, 0, 1.0
    elif isinstance(coarse, str):
        cptr, cny, cnx, rep, mult = None, 0, 0, -1, 1.0
    else:
        cfs, rep, mult = coarse
        assert all(cf.is_contiguous() and cf.dtype == torch.float32 for cf in cfs)
        cptr, (cny, cnx) = _lib.ptr_array(cfs), cfs[0].shape[:2]
    _lib.call("hhsr_align_level_batch", _lib.ptr(ref_lvl), rh, rw, rw, _lib.ptr(ref_hessian_lvl), _lib.ptr_array(movs),
              len(movs), mh, mw, mw, _lib.ptr_array(flows), ny, nx, ts, r, code, int(config.ica.tuning.n_iter), cptr,
              int(cny), int(cnx), int(rep), float(mult), _lib.stream())


def align_lvl(ref_lvl, tyled_pyr_lvl, ref_fft_lvl, ref_gradx_lvl, ref_grady_lvl, ref_hessian_lvl, moving_lvl,
              alignments, l, config):
    """Block matching then ICA on one level, in place on `alignments` (alignment.py:125-147).  For tiles up to 32 pixels
    both steps run in ONE fused kernel (config.hip.fused_align: false selects the two-kernel path, which is also what
    64-pixel tiles use)."""
    metric = config.block_matching.tuning.metrics[l]
    fl = _fused_level(l, config)
    if fl is not None:
        return _align_level_fused(fl, ref_lvl, ref_hessian_lvl, [moving_lvl], [alignments], None, config)
    if metric == "L2":
        align_lvl_block_matching_L2(ref_lvl, ref_fft_lvl, moving_lvl, alignments, l, config)
    elif metric == "L1":
        align_lvl_block_matching_L1(ref_lvl, moving_lvl, alignments, l, config)
    elif metric == "L1_ref_effective":
        align_lvl_block_matching_L1(ref_lvl, moving_lvl, alignments, l, config, effective=True)
    else:
        raise ValueError("Unknown block matching metric {}".format(metric))
    align_lvl_ica(ref_lvl, ref_gradx_lvl, ref_grady_lvl, ref_hessian_lvl, moving_lvl, alignments, l, config)


def align(ref_pyramid, tyled_pyr, ref_tiled_fft, ref_gradx, ref_grady, ref_hessian, img, config,
          moving_pyramid=None):
    """Coarse-to-fine alignment of one grey frame (alignment.py:84-123): align_batch() of one pyramid.  `moving_pyramid`:
    the frame's pyramid when the caller already built it (it does not depend on the reference frame)."""
    if moving_pyramid is None:
        moving_pyramid = build_gaussian_pyramid(_lib.f32c(img), config.block_matching.tuning.factors)
    return align_batch(ref_pyramid, ref_hessian, [moving_pyramid], config, ref_gradx, ref_grady)[0]


def _reads_coarse(l, config):
    """rep > 0 when level l's fused kernel can take its incoming flow straight from the coarser level (nearest-neighbour
    upscaling by `rep` fused into the launch: no separate upscaling launch), else 0.  Not for the coarsest level."""
    bm = config.block_matching.tuning
    q = bm.tile_sizes[l] // bm.tile_sizes[l + 1]
    if _fused_level(l, config) is None or q <= 0 or bm.flow_upscale_mode != "nearest":
        return 0
    return max(bm.factors[l + 1] // q, 0)


def can_align_batch(config):
    """Every level runs on the fused level kernel with the coarser flow read in place: align_batch() is then one launch
    per level for any number of frames."""
    n = len(config.block_matching.tuning.factors)
    return _fused_level(n - 1, config) is not None and all(_reads_coarse(l, config) > 0 for l in range(n - 1))


def align_batch(ref_pyramid, ref_hessian, moving_pyramids, config, ref_gradx=None, ref_grady=None):
    """Coarse-to-fine alignment of several frames against one reference pyramid; everything is enqueued on torch's current
    stream, no host synchronisation between levels (the reference needs a cuda.synchronize() per level to order its torch
    and Numba streams).  A level that runs on the fused kernel with the coarser flow read in place (or zero) is ONE launch
    for all frames (hhsr_align_level_batch) — the coarse levels are 7-27 us launches of a few hundred workgroups that
    cannot fill the GPU one frame at a time; with can_align_batch(config) that is every level.  Any other level runs frame
    by frame: upscale_lvl() or zeros, then align_lvl() (which needs `ref_gradx` / `ref_grady` for its two-kernel path).
    Returns the list of finest-level flow fields."""
    bm = config.block_matching.tuning
    n_lvl, nf = len(ref_pyramid), len(moving_pyramids)
    dev = moving_pyramids[0][0].device
    prev = None
    for i in range(n_lvl):
        l = n_lvl - i - 1
        ts = bm.tile_sizes[l]
        ny, nx = ref_pyramid[i].shape[0] // ts, ref_pyramid[i].shape[1] // ts
        movs = [p[i] for p in moving_pyramids]
        fl = _fused_level(l, config)
        rep = _reads_coarse(l, config) if prev is not None else 0
        if fl is not None and (prev is None or rep > 0):
            flows = list(torch.empty((nf, ny, nx, 2), dtype=torch.float32, device=dev).unbind(0))
            coarse = "zero" if prev is None else (prev, rep, float(bm.factors[l + 1]))
            _align_level_fused(fl, ref_pyramid[i], ref_hessian[i], movs, flows, coarse, config)
        else:
            flows = []
            for k, mov in enumerate(movs):
                flows.append(torch.zeros((ny, nx, 2), dtype=torch.float32, device=dev) if prev is None
                             else upscale_lvl(prev[k], (ny, nx), l, config))
                align_lvl(ref_pyramid[i], None, None, ref_gradx[i], ref_grady[i], ref_hessian[i], mov, flows[k], l, config)
        prev = flows
    return prev
