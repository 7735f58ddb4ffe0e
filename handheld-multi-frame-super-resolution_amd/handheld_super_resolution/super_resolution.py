"""Alg. 1 driver: main() and the process() facade (reference super_resolution.py:41-360).

MI355X design notes (vs the reference's per-frame Python loop):
  * everything is enqueued on ONE HIP stream (torch's current stream): no host synchronisation inside
    the hot path, no torch<->Numba stream fences;
  * each frame is uploaded once (the reference uploads it twice);
  * a frame's (raw, flow, covariances, robustness) stay resident in HBM (144 MB per 12 MP frame; a
    20-frame burst is <3 GB of the 288 GB) and the merge of the whole burst is ONE kernel with the
    accumulators in registers (merge.merge_burst), instead of a read-modify-write of the 2x576 MB
    accumulators per frame;
  * the front end (grey FFT, pyramid, alignment levels, raw pass) runs one launch per STAGE AND CHUNK of frames, chunks
    round-robin on two HIP streams (one for frames of 40 MP and more); bursts that start in host memory run as eager uploads + per-chunk HIP graphs
    (graph.HostBurstRunner), device-resident bursts as one graph per burst (graph.GraphRunner);
  * multi-GPU (distributed.py): alignment frame-parallel, one all-gather of the flow fields, robustness / kernels /
    merge row-parallel (default), or frames one per GPU with one reduce-scatter of the num / den accumulators.
"""
import atexit
import os
import threading
import time
from collections import namedtuple

import numpy as np
import torch

from . import _lib, raw2rgb
from .config import hip_opt, positive_int
from .noise_profile import estimate_noise_profile, noise_options
from .raw_frames import FLOAT, RawLayout, host_counts
from .utils_dng import dng_option, encode_dng, load_dng_burst
from .utils_image import (apply_orientation, compute_grey_images, compute_grey_images_batch, encode_image, encode_jpeg,
                          encode_png, frame_count_denoising_gauss, frame_count_denoising_median, frame_sharpness,
                          jpeg_option, png_option, robustness_mask)
from .white_balance import estimate_white_balance, wb_options
from .utils import divide, add, getTime, timer
from .alignment import init_alignment, build_gaussian_pyramids, align_batch, can_align_batch
from .params import sanitize_config, update_snr_config
from .robustness import (init_robustness, compute_robustness, compute_robustness_group, noise_curves_to_device, RobustnessSum,
                         ref_planes, upscale_warp_stats, mono_sigma_sq)
from .kernels import estimate_kernels, frame_stats, frame_stats_batch
from .merge import merge, merge_ref, merge_burst, can_fuse_acc_r, merge_fusions


def denoiser_enabled(config, store=True):
    """config.accumulated_robustness_denoiser.enabled is derived by process() upstream (super_resolution.py:291-296);
    derive it here too when main() is called directly (`store=False`: without writing it into the configuration)."""
    den = config.accumulated_robustness_denoiser
    if "enabled" in den:
        return bool(den.enabled)
    on = bool(den.median.enabled or den.gauss.enabled or den.merge.enabled)
    if store:
        den.enabled = on
    return on


def accumulation(config):
    """(denoiser_on, accumulate_r): the accumulated robustness is needed by the denoiser or asked for as a mask."""
    denoiser_on = denoiser_enabled(config)
    return denoiser_on, denoiser_on or bool(config.robustness.save_mask)


def main_plan(config, shape, n_comp, denoiser_on, accumulate_r):
    """main()'s path for a burst: (fused, batch, fuse_acc, fuse_min, den_fused).  fused: ONE merge launch (not with the
    denoiser); batch: the frames go through process_frames(), not the per-frame loop of the timers and debug copies;
    den_fused: the denoiser's form of both — one merge launch without the reference frame, the float64 robustness sum in
    one pass (it takes the 5x5 minimum on the way in: fuse_min whatever is accumulated), then merge_ref and divide."""
    fused_merge = bool(hip_opt(config, "fused_merge"))
    quiet = not (config.verbose >= 1 or bool(config.debug))
    fused = fused_merge and not denoiser_on
    den_fused = fused_merge and denoiser_on and can_fuse_acc_r(config) and n_comp > 0 and quiet
    batch = (fused and quiet) or den_fused
    fuse_acc, fuse_min = merge_fusions(config, shape, n_comp, accumulate_r and not den_fused, denoiser_on)
    return fused, batch, fused and fuse_acc, batch and fuse_min, den_fused


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("handheld_super_resolution (MI355X build): no HIP device is visible; this package has no "
                           "CPU path (the NumPy oracle under oracle/ is test infrastructure only)")
    return torch.device("cuda", torch.cuda.current_device())


ROB_GROUP = 4  # frames per robustness launch (hhsr_rob_frames)


def front_groups(k, batch, given, robustness, mono, batchable):
    """Sizes of the launch groups the front end runs for a chunk of k frames, `given` of which come with a flow field.
    The whole chunk is ONE group (one launch per stage) when the batched front end is on (BurstPipeline._batch) and either
    every flow is given — no alignment, one raw pass, which only the Bayer robustness path has in list form — or none is
    and every alignment level takes a list of frames (`batchable`: alignment.can_align_batch); else k groups of one."""
    whole = k >= 2 and batch and ((given == k and robustness and not mono) or (given == 0 and batchable))
    return [k] if whole else [1] * k


def _tensors(x):
    """All tensors in a nested tuple / list."""
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, (tuple, list)):
        for y in x:
            yield from _tensors(y)


DEFAULT_STREAMS = 2  # round 1, 12 MP x 20: 1 stream 15.3 ms, 2: 14.3, 3: 13.9, 4: 14.3 -> 3.  Round 6, with the batched front end and the
#                      graph-replayed step (four alternating bench runs each, one MI355X): 2 streams 7.70 - 7.80 ms, 3: 7.76 - 7.88
#                      (round 5's sweep had said the same: 8.21 against 8.36); eager, host-resident and denoiser legs the same or better
LARGE_FRAME = 40_000_000  # raw pixels from which the frame pipeline runs on ONE stream: every kernel of a 48 MP frame fills the
#                           GPU on its own and side streams only contend for the caches (round 6, one MI355X, 20 frames: 48 MP x3
#                           51.9 ms on one stream / 52.5 on three, 48 MP x2 32.4 / 32.7; 30 MP x2 21.7 / 21.2, 24 MP 17.9 / 17.1,
#                           12 MP 8.33 / 8.24: the smaller frames keep several)
_stream_pool = {}  # device index -> side streams, shared by all pipelines of the process


class _Staged:
    """A host frame whose upload is in flight on the upload stream: device tensor (dtype of the host frame) + event."""
    __slots__ = ("tensor", "event")

    def __init__(self, tensor, event):
        self.tensor, self.event = tensor, event


_upload_streams = {}  # device index -> the stream all prefetched uploads are queued on, in frame order


_LATE_FORK = os.environ.get("HHSR_LATE_FORK") is not None  # (read once) side streams fork behind the reference precompute:
# the way out of the early-fork ordering contract (BurstPipeline._on_streams)


class BurstPipeline:
    """Device-resident state of one burst: reference-frame precompute + per-frame stage chain."""

    def __init__(self, config, device=None):
        self.config = config
        self.device = device or _device()
        # `mode: grey` (monochrome sensors): the frames are their own grey images (super_resolution.py:106-109, 144-147),
        # one-channel robustness, per-pixel kernels, one-channel merge — the generic kernels of each stage
        self.mono = config.mode != "bayer"
        self.cfa = [[int(v) for v in row] for row in config.exif.cfa_pattern]
        self.wb = [float(v) for v in config.exif.white_balance]
        self.curves = noise_curves_to_device(config.noise_model.std_curve, config.noise_model.diff_curve, self.device)
        self.grey_method = config.grey_method
        self.ref = None
        self._streams = _stream_pool.setdefault(self.device.index, [])
        # validation hook (bench.py's parity attribution, tests): per-frame flow fields that replace align()
        self._inject_flows = hip_opt(config, "inject_flows")
        # frames given as integer sensor counts: {"black_levels": [R, G, B], "white_level": w} (see _ingest)
        self._raw_norm = hip_opt(config, "raw_norm")
        self._layouts = {}  # (dtype, shape) of an integer frame -> its RawLayout under raw_norm
        # (before, after): the flow fields handed to this pipeline are row slices (views) of larger fields with that many
        # tile rows around them — the sub-image pipelines of distributed.py; see robustness.compute_s
        self.flow_rows = (0, 0)
        # False: the side streams do not wait for the reference-frame events — the caller orders the reference precompute
        # before the frames itself (distributed.RowsPlan captures them as separate graphs: an event recorded in one
        # capture cannot be waited for in another)
        self.ref_wait = True
        # chunk-batched front end (one launch per stage for a chunk of frames, see front_groups); config.hip.batch: false
        # keeps the per-frame launches (A/B, tests), and so do the per-frame timers and the grey methods without a list form
        self._batch = bool(hip_opt(config, "batch")) and (self.mono or self.grey_method == "FFT") and config.verbose < 2

    def _ingest(self, img):
        """One frame -> float32 device tensor, on the current stream.  Float frames are the reference's call signature
        (normalised, white-balanced RAW).  Integer frames are sensor counts as the DNG holds them: they are uploaded as
        they are — half the PCIe bytes of the float32 frame — and normalised on the device with the reference loader's
        arithmetic (utils_dng.py:149-160, hhsr_normalize_raw_u16) using config.hip.raw_norm and config.exif.  With
        raw_norm["packing"] (a name of utils_dng.PACKINGS) and raw_norm["width"], uint8 frames [H, row_bytes] are the
        packed 10/12/14-bit counts themselves — 1.25 to 1.75 bytes per pixel over PCIe — and hhsr_normalize_raw_packed
        unpacks and normalises them in one pass."""
        staged = isinstance(img, _Staged)
        if staged:  # prefetch(): the copy was queued on the upload stream
            if img.event is not None:  # (None: a static staging buffer of graph.HostBurstRunner, ordered by the runner)
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(img.event)
                img.tensor.record_stream(cur)
            img = img.tensor
        t = img if torch.is_tensor(img) else torch.as_tensor(img)
        if t.dtype.is_floating_point:
            return _lib.f32c(t, self.device)
        if (t.is_cuda and not staged) or self._raw_norm is None:
            raise ValueError("integer frames are sensor counts: give config.hip.raw_norm = {black_levels, white_level} "
                             "(host arrays), or pass normalised float frames")
        key = (t.dtype, t.shape)
        layout = self._layouts.get(key)
        if layout is None:  # (once per frame shape: the packed row length is a call into the library)
            layout = self._layouts[key] = RawLayout.from_raw_norm(self._raw_norm, t)
        return layout.normalize(t, self.wb, self.cfa, self.device)

    def prefetch(self, imgs):
        """Queue the uploads of all page-locked host frames of a list NOW, back to back on one upload stream, instead of
        one by one as the host gets to each frame's kernels: enqueuing a frame's ~13 launches takes the host longer
        (0.5-0.7 ms) than the copy engine needs for the frame (0.43 ms for 24 MB of uint16 counts), so host-paced
        uploads leave the link idle half of the time (measured: last copy done at 13.9 ms instead of 8.5).  Frames in
        pageable memory keep the per-frame order (their copies block the host; the GPU works on frame i meanwhile)."""
        out, stream = [], None
        for img in imgs:
            t = img if torch.is_tensor(img) else (torch.as_tensor(img) if isinstance(img, np.ndarray) else None)
            if t is None or t.is_cuda or not t.is_pinned():
                out.append(img)
                continue
            if stream is None:
                stream = _upload_streams.get(self.device.index)
                if stream is None:
                    # (high priority = its own hardware queue: see graph.HostBurstRunner)
                    from .graph import shared_streams

                    stream = _upload_streams[self.device.index] = shared_streams(self.device)[1]
            if t.dtype == torch.float64:  # (half the PCIe bytes: the kernels work on float32 frames anyway)
                t = t.to(torch.float32).pin_memory()
            with torch.cuda.stream(stream):
                d = t.contiguous().to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
            self._last_upload = ev
            out.append(_Staged(d, ev))
        return out

    def uploads_done(self):
        """Block until the last queued upload has left the host: the caller's page-locked buffers may be refilled."""
        ev = getattr(self, "_last_upload", None)
        if ev is not None:
            ev.synchronize()
            self._last_upload = None

    def _timed(self, func, level, start_s=None, end_s=None):
        """The reference's per-stage timers (super_resolution.py:72-81): synchronising wall-clock wrappers, active from
        config.verbose >= level (2: stages, 3: grey images), plain function otherwise."""
        return timer(func, self.config.verbose >= level, start_s, end_s)

    def init_ref(self, ref_img, alignment=True, robustness=True):
        """Reference-frame precompute.  `alignment=False` / `robustness=False` skip the halves the multi-GPU
        path does not need on a given pipeline (distributed.py: whole-frame alignment state vs the sub-image's
        robustness / kernel state)."""
        with torch.cuda.device(self.device):  # every launch below goes to this device's current stream
            return self._init_ref(ref_img, alignment, robustness)

    def _init_ref(self, ref_img, alignment, robustness):
        cfg = self.config
        main = torch.cuda.current_stream(self.device)
        self._entry = torch.cuda.Event()  # everything the caller enqueued before (e.g. the frames' upload) is done
        self._entry.record(main)
        self._entry_fresh = True  # the next _on_streams() forks its side streams HERE, not behind the reference precompute
        self.ref = self._ingest(ref_img)
        self.align_state = self.grey_ref = None
        if alignment:
            sanitize_config(cfg, tuple(self.ref.shape))
            grey = self.ref if self.mono else self._timed(
                compute_grey_images, 3, end_s="- Ref grey image estimated by {}".format(self.grey_method))(
                self.ref, self.grey_method)
            self.align_state = self._timed(init_alignment, 2, "\nInitializing alignment", "Alignment initialized (Total)")(
                grey, cfg)
            self.grey_ref = grey
        # two milestones of the reference precompute: the frames' alignment only needs the first (grey image, pyramid,
        # gradients, Hessians: ~0.25 ms); the robustness state behind it (raw pass + upsampled planes, another ~0.25 ms)
        # is first needed after a frame's alignment and raw pass — the side streams do not sit out the second half
        # (measured: no change of the 12 MP step, the other frames' FFTs already fill that time; kept for short bursts)
        self._align_ready = torch.cuda.Event()
        self._align_ready.record(main)
        self.ref_means = self.ref_vars = self.ref_covs = self.ref_sigma_sq = None
        if robustness and cfg.robustness.enabled and self.mono:
            m, v, self.ref_covs = self._timed(frame_stats, 2, "\nEstimating ref image local stats + kernels",
                                              "Local stats + kernels estimated (Total)")(
                self.ref, self.cfa, self.wb, cfg, want_vars=True)
            self.ref_means, self.ref_vars = upscale_warp_stats(m), upscale_warp_stats(v)
            self.ref_sigma_sq = mono_sigma_sq(self.ref_means, self.ref_vars, self.curves[0])
        elif robustness and cfg.robustness.enabled:  # init_robustness + the reference frame's kernels from one raw pass,
            # then the upsampled means, sigma^2 and curve indices from one pass over the guide statistics
            m, v, self.ref_covs = self._timed(frame_stats, 2, "\nEstimating ref image local stats + kernels",
                                              "Local stats + kernels estimated (Total)")(
                self.ref, self.cfa, self.wb, cfg, want_vars=True)
            self.ref_means, self.ref_sigma_sq = ref_planes(m, v, self.curves[0])
            self.ref_vars = None  # only needed for sigma^2, which is already there
        elif robustness:
            self.ref_means, self.ref_vars = init_robustness(self.ref, self.cfa, self.wb, cfg)
            self.ref_covs = estimate_kernels(self.ref, cfg)
        self._ref_ready = torch.cuda.Event()
        self._ref_ready.record(main)
        return self

    def flow_grid(self):
        """(ny, nx) of the flow field: tiles of the (padded) finest reference level."""
        lvl0 = self.align_state[0][-1]
        ts = int(self.config.block_matching.tuning.tile_size)
        return lvl0.shape[0] // ts, lvl0.shape[1] // ts

    def align_frames(self, comp_imgs, n_streams=None):
        """Flow fields float32 [ny, nx, 2] of a list of frames (grey -> pyramid -> coarse-to-fine alignment): chunks of
        frames round-robin on the side streams (like process_frames)."""
        with torch.cuda.device(self.device):
            comp_imgs = self.prefetch([comp_imgs[i] for i in range(len(comp_imgs))])
            chunks = self._chunks(len(comp_imgs), n_streams)
            out = self._on_streams(len(chunks), n_streams, False,
                                   lambda ci, wait: self._grouped(comp_imgs, wait, chunks[ci], None, stats=False))
            return [f for chunk in out for f in chunk]

    def _grouped(self, imgs, wait_ref, indices, flows, stats=True):
        """_front_group() of the frames `indices` of a burst, in the launch groups of front_groups().  `flows`: flow fields
        of the burst's frames that replace their alignment (None, or None for a frame: aligned here)."""
        fl = [None if flows is None else flows[i] for i in indices]
        groups = front_groups(len(indices), self._batch, sum(f is not None for f in fl), bool(self.config.robustness.enabled),
                              self.mono, can_align_batch(self.config))
        out, i0 = [], 0
        for k in groups:
            out += self._front_group([imgs[i] for i in indices[i0:i0 + k]], wait_ref, fl[i0:i0 + k], stats)
            i0 += k
        return out

    def _front_group(self, imgs, wait_ref, flows, stats=True):
        """The front end of n >= 1 frames, one launch per stage: ingest, then grey -> pyramid -> alignment (or the given
        `flows`: all or none), then guide means + kernel covariances.  Returns a list of (raw, flow, covs, guide means or
        None), with `stats=False` of flows.  With the default configuration (Bayer frames, FFT grey image, fused level
        kernels) that is 3 transform phases, 3 pyramid levels, 4 alignment levels, 1 raw pass: 11 launches per group instead
        of per frame, and the latency-bound stages (FFT phases, coarse pyramid / alignment levels: a few hundred workgroups
        per frame) see enough work to fill the GPU.  Results per frame do not depend on the grouping (tests: batch == single)."""
        cfg = self.config
        raws = [self._ingest(img) for img in imgs]
        if flows[0] is not None:  # (nothing here needs the reference frame: the caller waits before the robustness)
            flows = [_lib.f32c(f, self.device) for f in flows]
        else:
            greys = raws if self.mono else self._timed(  # mono: the frame itself
                compute_grey_images_batch, 3, end_s="- grey images estimated by {}".format(self.grey_method))(raws, self.grey_method)
            pyramids = build_gaussian_pyramids(greys, cfg.block_matching.tuning.factors)
            if wait_ref is not None:
                torch.cuda.current_stream(self.device).wait_event(self._align_ready)
            st = self.align_state
            flows = self._timed(align_batch, 2, "\nBeginning alignment", "Image aligned (Total)")(
                st[0], st[5], pyramids, cfg, st[3], st[4])
        if not stats:
            return flows
        if not cfg.robustness.enabled:
            est = self._timed(estimate_kernels, 2, "\nEstimating kernels", "Kernels estimated (Total)")
            return [(raw, f, est(raw, cfg), None) for raw, f in zip(raws, flows)]
        # guide means + kernel covariances from one pass over the raw frames (mono: per-pixel covariances, frame by frame)
        stat = self._timed(frame_stats if self.mono else frame_stats_batch, 2, "\nEstimating kernels + guide statistics",
                           "Kernels + guide statistics estimated (Total)")
        sts = [stat(raw, self.cfa, self.wb, cfg) for raw in raws] if self.mono else stat(raws, self.cfa, self.wb, cfg)
        return [(raw, f, st[2], st[0]) for raw, f, st in zip(raws, flows, sts)]

    def _robustness(self, fronts, accumulate_r=None, fuse_local_min=False):
        """Robustness of a group of frames of the burst (one launch per 4 frames shares the pass over the
        reference-frame planes): list of (raw, flow, covs, r)."""
        cfg = self.config
        if not cfg.robustness.enabled or len(fronts) == 1 or self.mono:
            rob = self._timed(compute_robustness, 2, "\nEstimating robustness", "Robustness estimated (Total)")
            return [(raw, flow, covs,
                     rob(raw, self.ref_means, self.ref_vars, flow, self.cfa, self.wb, self.curves, cfg,
                                        accumulate_into=accumulate_r, ref_sigma_sq=self.ref_sigma_sq, comp_means=means,
                                        fuse_local_min=fuse_local_min and cfg.robustness.enabled,
                                        flow_rows=self.flow_rows))
                    for raw, flow, covs, means in fronts]
        rs = compute_robustness_group([f[0] for f in fronts], self.ref_means, [f[1] for f in fronts], self.curves, cfg,
                                      self.ref_sigma_sq, [f[3] for f in fronts], accumulate_into=accumulate_r,
                                      fuse_local_min=fuse_local_min, flow_rows=self.flow_rows)
        return [(f[0], f[1], f[2], r) for f, r in zip(fronts, rs)]

    def process_frame(self, img, accumulate_r=None, wait_ref=None, fuse_local_min=False, index=None, flow=None):
        """grey -> kernels -> align -> robustness for one comp frame; returns (raw, flow, covs, r).
        `accumulate_r`: optional float32 [H, W] that receives += r (fused into the local-min pass).
        `wait_ref`: event after which the reference-frame state is complete — the frame's own grey image and
        pyramid do not need it and are enqueued before the wait, so on a side stream they overlap the
        (latency-bound) reference precompute.
        `flow`: a flow field that replaces the alignment (multi-GPU step B; validation hook
        config.hip.inject_flows via `index`)."""
        if flow is None and self._inject_flows is not None and index is not None:
            flow = self._inject_flows[index]
        fronts = self._front_group([img], wait_ref, [flow])
        if wait_ref is not None:
            torch.cuda.current_stream(self.device).wait_event(wait_ref)
        return self._robustness(fronts, accumulate_r, fuse_local_min)[0]

    def process_frames(self, comp_imgs, accumulate_r=None, n_streams=None, fuse_local_min=False, flows=None):
        """process_frame() over a list of frames.  Frames are independent until the merge, so they are
        issued round-robin on `n_streams` HIP streams (config.hip.streams, default 2; 1 for frames >= LARGE_FRAME): the launch-latency-
        bound coarse pyramid levels of one frame overlap the bandwidth-bound kernels of another.  The caller's
        stream waits for all of them before returning.  A per-frame `accumulate_r` (read-modify-write of one
        map) forces a single stream.  `flows`: per-frame flow fields that replace the alignment."""
        with torch.cuda.device(self.device):
            n = len(comp_imgs)
            comp_imgs = self.prefetch(comp_imgs)
            chunks = self._chunks(n, n_streams)
            if flows is None:
                flows = self._inject_flows

            def work(ci, wait):
                fronts = self._grouped(comp_imgs, wait, chunks[ci], flows)
                if wait is not None:  # the robustness needs the second half of the reference precompute
                    torch.cuda.current_stream(self.device).wait_event(wait)
                return self._robustness(fronts, accumulate_r if wait is None else None, fuse_local_min)

            out = self._on_streams(len(chunks), n_streams, accumulate_r is not None, work)
            return [f for chunk in out for f in chunk]

    def _chunks(self, n, n_streams=None):
        """Frame indices per chunk.  Chunks of up to `config.hip.chunk` (default ROB_GROUP) frames stay together on a
        stream: their robustness is one launch per ROB_GROUP frames that reads the reference-frame planes once
        (hhsr_rob_frames), and with the batched front end every stage is one launch per chunk; chunk sizes are balanced
        over the streams."""
        streams = self._n_streams(n_streams)
        size = self._chunk_size()
        n_chunks = min(n, streams * -(-n // (streams * size))) if n else 0
        chunks, i = [], 0
        for c in range(n_chunks):
            k = n // n_chunks + (1 if c < n % n_chunks else 0)
            chunks.append(list(range(i, i + k)))
            i += k
        return chunks

    def _chunk_size(self):
        chunk = hip_opt(self.config, "chunk")
        return max(1, min(ROB_GROUP if chunk is None else int(chunk), _lib.MAX_BATCH))

    def _n_streams(self, n_streams):
        if n_streams is None:
            n_streams = hip_opt(self.config, "streams")
        if n_streams is None:
            n_streams = 1 if self.ref is not None and self.ref.numel() >= LARGE_FRAME else DEFAULT_STREAMS
        return max(1, int(n_streams))

    def _on_streams(self, n, n_streams, serial, work):
        """work(i, wait_event) for i < n; on one stream (wait_event None) or round-robin on the side streams."""
        n_streams = self._n_streams(n_streams)
        # Round 5: the side streams fork at the START of the reference precompute (self._entry), not behind it: a frame's own
        # grey image and pyramid do not need the reference frame, the alignment waits for _align_ready, the robustness
        # for `entry` below (the whole precompute and whatever else the caller's stream holds).  Until now the fork event
        # was recorded here, i.e. behind the ~0.5 ms of single-frame, latency-bound reference kernels — 6 % of the 12 MP
        # step, a sixth of a rank's step on 8 GPUs — and the _align_ready / _ref_ready waits had nothing left to wait for.
        # CONTRACT of the early fork: the side streams are ordered behind the caller's stream as of the START of
        # init_ref only.  Whatever the caller enqueues on its stream between init_ref() and this call — producing or
        # normalising comp frames on the device, a flow field that needs a copy — is NOT ordered before the side streams'
        # first reads; the in-repo callers hand over inputs that predate init_ref (or staged / host frames) and contiguous
        # float32 flow views.  HHSR_LATE_FORK=1 restores the fork at this call for callers that cannot promise that.
        early = bool(self.ref_wait and getattr(self, "_entry_fresh", False) and n_streams > 1 and not serial and n >= 1
                     and not _LATE_FORK)
        self._entry_fresh = False
        if not early and (n_streams <= 1 or serial or n < 2):
            return [work(i, None) for i in range(n)]
        main = torch.cuda.current_stream(self.device)
        if len(self._streams) < n_streams:
            self._streams += [torch.cuda.Stream(self.device) for _ in range(n_streams - len(self._streams))]
        pool = self._streams[:n_streams]
        # everything the caller enqueued so far (frame uploads / normalisation, a previous call's merge that still
        # reads buffers the allocator may hand out again) is ordered before the side streams' work
        entry = torch.cuda.Event()
        entry.record(main)
        for s in pool:
            s.wait_event(self._entry if early else entry)
        results = []
        for i in range(n):
            s = pool[i % n_streams]
            with torch.cuda.stream(s):
                f = work(i, entry if early else (self._ref_ready if self.ref_wait else None))
            for t in _tensors(f):
                t.record_stream(main)  # consumed by the merge on the caller's stream (raw too: it is allocated on
                # the side stream when the frame was uploaded / converted there)
            results.append(f)
        for s in pool:
            main.wait_stream(s)
        return results

    def output_size(self):
        s = self.config.scale
        H, W = self.ref.shape
        return round(s * H), round(s * W)


_main_runners = []  # [(config, ConfigWatch, HostBurstRunner)], most recently used last
_main_runners_lock = threading.Lock()  # main() may be called from several threads


def _drop_host_runners():
    """Interpreter exit: release the cached runners (HIP graphs, page-locked staging, copy threads) while the HIP runtime
    is still up instead of in whatever order module teardown picks."""
    while _main_runners:
        _, _, runner = _main_runners.pop()
        runner.close()


atexit.register(_drop_host_runners)


def _host_runner(config, device):
    """The HostBurstRunner of a configuration object that main() is called with again and again (a serving loop); a
    configuration edited in place gets a new one.  At most two are kept (each holds a burst's intermediates)."""
    from .graph import ConfigWatch, HostBurstRunner

    with _main_runners_lock:
        for k, (cfg, watch, runner) in enumerate(_main_runners):
            if cfg is config and runner.device == device:
                _main_runners.append(_main_runners.pop(k))
                if watch.changed(config):
                    _main_runners.pop()
                    break
                return runner
        watch = ConfigWatch()
        watch.changed(config)
        runner = HostBurstRunner(config, device)
        _main_runners.append((config, watch, runner))
        while len(_main_runners) > 2:
            _main_runners.pop(0)[2].close()
        return runner


def main(ref_img, comp_imgs, config, *, _no_runner=False):
    """Alg. 1 (reference super_resolution.py:41-200).

    ref_img [H, W], comp_imgs [N-1, H, W]: float32 NumPy arrays (as in the reference) or torch tensors
    (host or already device-resident).  Returns (num, debug_dict): num is the normalised RGB image,
    a float32 GPU tensor [sH, sW, 3] WITHOUT post-processing; debug_dict has 'flow' / 'robustness' lists
    (NumPy, only if config.debug) and 'accumulated robustness' (GPU tensor) when the mask is requested.

    Host-resident bursts (the reference's signature) that come back with the same configuration object, shapes and
    dtype — a serving loop — run through graph.HostBurstRunner from the third call on: uploads as eager copies, the
    kernels as per-chunk HIP graphs, bit-identical results; main() then returns when the host buffers may be refilled
    (all uploads done) and hands out fresh tensors like the reference (one device copy of the result).
    `config.hip.graph: false` keeps the eager path."""
    if not _no_runner and torch.cuda.is_available():
        from .graph import HostBurstRunner

        denoiser_enabled(config)  # derives den.enabled in place NOW: the runner's ConfigWatch snapshot then already has it
        if HostBurstRunner.usable(config, ref_img, comp_imgs):
            # (the runner keeps a burst's staging and intermediates on the device — ~6 GB at 12 MP x 20, plus 1.6 GB for the
            # chained merge of float bursts — until the configuration object is dropped or edited; config.hip.graph: false
            # opts out.)  The result is cloned inside the runner's lock: concurrent callers never see each other's pixels
            return _host_runner(config, _device()).call_cloned(ref_img, comp_imgs)
    verbose = config.verbose >= 1
    debug_mode = bool(config.debug)
    debug_dict = {"robustness": [], "flow": []}
    denoiser_on, accumulate_r = accumulation(config)

    if verbose:
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        print("\nProcessing reference image ---------\n")
    pipe = BurstPipeline(config).init_ref(ref_img)
    dev = pipe.device
    H, W = pipe.ref.shape
    sH, sW = pipe.output_size()
    fused, batch, fuse_acc, fuse_min, den_fused = main_plan(config, (H, W), len(comp_imgs), denoiser_on, accumulate_r)
    # the denoiser DECIDES on the accumulated robustness: float64 sum like the reference's (robustness.RobustnessSum); a sum
    # that is only reported (save_mask) stays the float32 sum of the kernels
    acc_sum = RobustnessSum((H, W), dev) if denoiser_on else None
    accumulated_r = torch.zeros((H, W), dtype=torch.float32, device=dev) if (accumulate_r and not denoiser_on) else None
    num = torch.empty((sH, sW, 3), dtype=torch.float32, device=dev)
    den = None
    if den_fused:
        den = torch.empty_like(num)
    elif not fused:
        num.zero_()
        den = torch.zeros_like(num)
    if verbose:
        torch.cuda.synchronize()
        getTime(t1, "\nRef Img processed (Total)")

    frames = []
    n_images = len(comp_imgs)
    if batch:
        # the x2 / x3 merge kernels take the 5x5 local minimum of the robustness themselves (one pass and 8 B/pixel less
        # per frame); a separately accumulated robustness map needs the filtered maps
        # (page-locked host frames: all uploads are queued now, back to back — BurstPipeline.prefetch)
        frames = pipe.process_frames([comp_imgs[i] for i in range(n_images)], None if fuse_acc else accumulated_r,
                                     fuse_local_min=fuse_min)
        if den_fused:  # the float64 sum takes the minimum on the way in (HHSR_ROB_SUM_MIN5): the filtered maps are never written
            acc_sum.add_many([f[3] for f in frames], unfiltered=fuse_min)
        n_images = 0  # the per-frame loop below is the verbose / debug / sequential-merge path
    for im_id in range(n_images):
        if verbose:
            torch.cuda.synchronize()
            print("\nProcessing image {} ---------\n".format(im_id + 1))
            im_time = time.perf_counter()
        raw, flow, covs, r = pipe.process_frame(comp_imgs[im_id], None if fuse_acc else accumulated_r, index=im_id)
        if acc_sum is not None:
            acc_sum.add(r)
        if fused:
            frames.append((raw, flow, covs, r))
        else:
            pipe._timed(merge, 2, "\nAccumulating Image", "Image accumulated (Total)")(raw, flow, covs, r, num, den, pipe.cfa,
                                                                                          config)
        if debug_mode:  # the reference crashes here at HEAD (Tensor.copy_to_host)
            debug_dict["flow"].append(flow.cpu().numpy())
            debug_dict["robustness"].append(r.cpu().numpy())
        if verbose:
            torch.cuda.synchronize()
            getTime(im_time, "\nImage processed (Total)")

    ref_covs = pipe.ref_covs
    if fused:
        pipe._timed(merge_burst, 2, "\nAccumulating all frames + ref Img + normalising", "Burst merged (Total)")(
            frames, pipe.ref, ref_covs, num, None, pipe.cfa, config, do_ref=True, divide=True,
            acc_r=accumulated_r if fuse_acc else None, local_min=fuse_min)
    else:
        if den_fused:
            merge_burst(frames, None, None, num, den, pipe.cfa, config, do_ref=False, divide=False, store_den=True,
                        local_min=fuse_min)
        dec = acc_sum.for_decisions(config.accumulated_robustness_denoiser.merge.max_frame_count) if denoiser_on else None
        if den_fused:  # reference frame + normalisation in ONE pass over the accumulators (HHSR_REF_DIVIDE), float32 weights
            # where the denoiser does not widen (HHSR_REF_FAST: the arithmetic of the fused merge's reference frame)
            merge_ref(pipe.ref, ref_covs, num, den, pipe.cfa, config, dec, divide=True, fast=True)
        else:
            pipe._timed(merge_ref, 2, "\nAccumulating ref Img", "Ref Img accumulated (Total)")(
                pipe.ref, ref_covs, num, den, pipe.cfa, config, dec)
            pipe._timed(divide, 2, end_s="\n------------------------\nImage normalized (Total)")(num, den)
    if verbose:
        torch.cuda.synchronize()
        s = "\nTotal ellapsed time : "
        print(s, " " * (50 - len(s)), ": ", round((time.perf_counter() - t1), 2), "seconds")
    if accumulate_r:
        debug_dict["accumulated robustness"] = acc_sum.mask() if denoiser_on else accumulated_r
    # host-buffer contract: main() returns when the caller's (page-locked) frames have been read — the uploads were
    # queued asynchronously (BurstPipeline.prefetch) and a serving loop refills its staging buffers right after the
    # call; the kernels keep running asynchronously on the current stream as before
    pipe.uploads_done()
    return num, debug_dict


REFERENCE_SELECT = ("first", "sharpest")
REFERENCE_CANDIDATES = 3  # HDR+ picks among the first three frames: a later base frame costs shutter lag


def reference_options(config):
    """(select, candidates) of the optional section config.reference = {"select": "first" | "sharpest", "candidates": 3}
    (not in the reference schema, like config.output; absent: ("first", 3)).  ValueError for anything else."""
    sec = config.get("reference", None) or {}
    select = str(sec.get("select", "first"))
    if select not in REFERENCE_SELECT:
        raise ValueError(f"config.reference.select {select!r}: first or sharpest")
    return select, positive_int("reference", "candidates", sec.get("candidates", REFERENCE_CANDIDATES))


def candidate_count(config, n_burst):
    """How many of a burst's n_burst frames are candidates: config.reference.candidates clamped to the burst's length."""
    return max(1, min(reference_options(config)[1], int(n_burst)))


def pick_reference(scores):
    """Index of the largest finite score, ties to the lowest index; a non-finite score never wins; 0 if none is finite."""
    best, arg = -np.inf, 0
    for i, s in enumerate(np.asarray(scores, np.float64).reshape(-1)):
        if np.isfinite(s) and s > best:
            best, arg = s, i
    return arg


def select_reference(ref, comp, config, cfa_pattern=None, layout=RawLayout(FLOAT)):
    """(index, scores): the sharpest of the burst's first config.reference.candidates frames (clamped to the burst's
    length), [ref, comp[0], ..., comp[K - 2]] in burst order, scored on the GPU by utils_image.frame_sharpness; `index` by
    pick_reference, `scores` a float64 ndarray [K].  Host frames are uploaded in their own form — float32, uint16 counts
    or, with the RawLayout of a packed burst, the packed uint8 rows — and scored as they are: integer counts are not
    normalised first.  `cfa_pattern`: the burst's (default: config.exif's); ignored with `mode: grey`, whose score has no
    CFA.  One host synchronisation (the scores decide what is uploaded and merged next)."""
    k = candidate_count(config, 1 + len(comp))
    dev = _device()
    frames = [layout.upload(f, dev) for f in [ref] + [comp[i] for i in range(k - 1)]]
    cfa = None if config.mode == "grey" else np.asarray(config.exif.cfa_pattern if cfa_pattern is None else cfa_pattern).tolist()
    scores = frame_sharpness(frames, cfa, packing=layout.packing, width=layout.width).cpu().numpy()
    return pick_reference(scores), scores


def reorder_burst(ref, comp, index):
    """(ref, comp) with frame `index` of [ref, comp[0], ...] as the reference frame; the other frames keep their order."""
    if index == 0:
        return ref, comp
    j = index - 1
    if torch.is_tensor(comp):
        return comp[j], torch.cat([torch.as_tensor(ref).to(comp)[None], comp[:j], comp[j + 1:]])
    if isinstance(comp, np.ndarray):
        return comp[j], np.concatenate([np.asarray(ref, dtype=comp.dtype)[None], comp[:j], comp[j + 1:]])
    comp = list(comp)
    return comp[j], [ref] + comp[:j] + comp[j + 1:]


def _first_frames(ref_raw, raw_comp, n_frames):
    """The reference frame and the next n_frames - 1 frames of the burst (clamped to its length)."""
    return [ref_raw] + [raw_comp[i] for i in range(max(1, min(int(n_frames), 1 + len(raw_comp))) - 1)]


def estimate_burst_profile(ref_raw, raw_comp, burst, layout, config, n_frames=1, min_tiles=16):
    """The noise profile of a burst (noise_profile.estimate_noise_profile) from its reference frame `ref_raw`, already
    normalised, and with n_frames > 1 from the next n_frames - 1 frames of `raw_comp` as well (clamped to the burst's length);
    integer frames are normalised like the reference frame, by the burst's RawLayout.  `mode: grey`: no CFA, unit gains."""
    frames = [layout.normalize(np.asarray(f), burst["white_balance"], burst["cfa_pattern"]) if i and host_counts(f) else f
              for i, f in enumerate(_first_frames(ref_raw, raw_comp, n_frames))]
    cfa_wb = (None, None) if config.mode == "grey" else (np.asarray(burst["cfa_pattern"]).tolist(),
                                                         [float(v) for v in list(burst["white_balance"])[:3]])
    return estimate_noise_profile(frames, *cfa_wb, min_tiles)


def estimate_burst_white_balance(ref_raw, raw_comp, burst, layout, n_frames=1, min_tiles=16):
    """The white balance of a burst of integer counts (white_balance.estimate_white_balance) from its reference frame
    `ref_raw` and, with n_frames > 1, from the next n_frames - 1 frames of `raw_comp` as well (clamped to the burst's
    length): uint16 counts or, by the burst's RawLayout, packed rows, uploaded and measured as they are."""
    return estimate_white_balance(_first_frames(ref_raw, raw_comp, n_frames), np.asarray(burst["cfa_pattern"]).tolist(),
                                  layout.black_levels, layout.white_level, layout.packing, layout.width, min_tiles)


def prepare_config(config, ref_raw, alpha=None, beta=None, cfa_pattern=None, white_balance=None, iso=100,
                   std_curve=None, diff_curve=None, shape=None):
    """The parameter derivation process() performs between loading the burst and calling main()
    (reference super_resolution.py:227-296): noise model, SNR -> tile size / merge tunings, sanity
    checks, exif block, denoiser switch.  Mutates `config` in place like the reference."""
    from .synthetic import noise_curves

    if config.noise_model.get("alpha", None) is not None:
        alpha, beta = config.noise_model.alpha, config.noise_model.beta
    if alpha is None or beta is None:
        raise ValueError("noise model (alpha, beta) missing: give it in config.noise_model or in the burst")
    config.noise_model.update({"alpha": float(alpha), "beta": float(beta)})
    if std_curve is None or diff_curve is None:
        # the reference draws these by an unseeded Monte-Carlo (fast_monte_carlo.py); here: its analytic
        # un-clipped limit (synthetic.noise_curves) unless the caller supplies curves
        std_curve, diff_curve = noise_curves(float(alpha), float(beta))
    brightness = float(ref_raw.mean()) if torch.is_tensor(ref_raw) else float(np.mean(ref_raw))
    id_noise = min(max(round(1000 * brightness), 0), len(std_curve) - 1)
    SNR = brightness / float(std_curve[id_noise])
    if config.verbose >= 1:
        print(" ", 10 * "-")
        print("|ISO : {}".format(iso))
        print("|Image brightness : {:.2f}".format(brightness))
        print("|expected noise std : {:.2e}".format(float(std_curve[id_noise])))
        print("|Estimated SNR : {:.2f}".format(SNR))
    update_snr_config(config, SNR)
    sanitize_config(config, tuple(shape if shape is not None else ref_raw.shape))
    config.exif = {"cfa_pattern": np.asarray(cfa_pattern).tolist(), "iso": iso,
                   "white_balance": [float(v) for v in white_balance]}
    config.noise_model.update({"std_curve": np.asarray(std_curve).tolist(), "diff_curve": np.asarray(diff_curve).tolist()})
    den = config.accumulated_robustness_denoiser
    den.enabled = bool(den.median.enabled or den.gauss.enabled or den.merge.enabled)
    return config


OutputOptions = namedtuple("OutputOptions", "format dtype quality restart_mcus subsampling huffman filter interval_bytes "
                                            "tile predictor", defaults=(None,) * 8)
IntakeOptions = namedtuple("IntakeOptions", "ref_select noise_source noise_frames noise_min_tiles wb_source wb_frames wb_min_tiles")


def output_options(config):
    """The optional section ``config.output`` (not in the reference schema) as an OutputOptions (None: a key the format does
    not read); anything it cannot hold is a ValueError here, before the burst is touched, not after it has been merged.
    ``config.output = {"dtype": "uint8" | "uint16"}`` (absent or "float32": the float32 image): the finished, oriented image
    is quantised on the GPU — rint(clip(nan_to_num(x), 0, 1) * M), half to even, M = 255 / 65535: skimage's img_as_ubyte and
    the reference's 16-bit TIFF rule (hhsr_encode_image) — and only the integer image is copied; the result is an ndarray of
    that dtype, [sH, sW, 3] or, with ``mode: grey``, [sH, sW] (channel 0).
    ``config.output = {"format": "jpeg", "quality": 90, "restart_mcus": ...}`` (``format`` absent or "raw": everything above,
    unchanged): the result is instead the complete baseline JPEG file of the uint8 image as a 1-D uint8 ndarray, coded on the
    GPU (utils_image.encode_jpeg; one component with ``mode: grey``; write it with utils_image.save_jpeg).  ``dtype`` may be
    absent or "uint8" then, anything else is a ValueError.  ``subsampling: 444 | 420`` (string or integer; 420 halves the
    chroma planes and is refused with ``mode: grey``) and ``huffman: standard | optimized`` (tables made for the image: a
    smaller file for one more synchronisation) choose the encoder's options; both keys are read only with ``format: jpeg``,
    anything else is a ValueError.
    ``config.output = {"format": "png", "dtype": "uint8" | "uint16", "filter": ..., "interval_bytes": ...}``: the result is
    the complete PNG file of the uint8 (default) or uint16 image as a 1-D uint8 ndarray, filtered and deflate-coded on the
    GPU (utils_image.encode_png; colour type 0 with ``mode: grey``; write it with utils_image.save_png_bytes).  ``filter``:
    none | sub | up | average | paeth | adaptive (default); ``interval_bytes``: 1 .. 2^20 (default
    utils_image.PNG_INTERVAL_BYTES).  ``dtype: float32``, another filter name or interval is a ValueError.
    ``config.output = {"format": "dng", "tile": ..., "predictor": ...}``: the result is the complete LinearRaw DNG file of the
    uint16 image as a 1-D uint8 ndarray, its lossless-JPEG tiles coded on the GPU (utils_dng.encode_dng; one sample per
    pixel with ``mode: grey``; write it with utils_dng.save_dng_bytes).  ``tile``: one integer or [h, w], multiples of 16 in
    16 .. 65535 (default utils_dng.DNG_TILE); ``predictor``: 1 .. 7 (default 1); ``dtype`` may be absent or "uint16".  A DNG
    holds the linear image: ``postprocessing.enabled: true`` with it is a ValueError, and the image is not rotated — the
    burst's orientation goes into the file's Orientation tag (finish)."""
    sec = config.get("output", None) or {}
    fmt = str(sec.get("format", "raw"))
    if fmt == "dng":
        dtype = str(sec.get("dtype", "uint16"))
        if dtype != "uint16":
            raise ValueError(f"config.output.format dng holds 16-bit samples: output.dtype {dtype!r} contradicts it")
        tile, predictor = dng_option("tile", _plain(sec.get("tile", None))), dng_option("predictor", sec.get("predictor", None))
        if config.postprocessing.enabled:
            raise ValueError("config.output.format dng holds the linear image: switch post-processing off "
                             "(postprocessing.enabled: false)")
        return OutputOptions(fmt, dtype, tile=tile, predictor=predictor)
    if fmt not in ("raw", "jpeg", "png"):
        raise ValueError(f"config.output.format {fmt!r}: raw, jpeg or png")
    dtype = str(sec.get("dtype", "uint8" if fmt in ("jpeg", "png") else "float32"))
    if dtype not in ("float32", "uint8", "uint16"):
        raise ValueError(f"config.output.dtype {dtype!r}: float32, uint8 or uint16")
    if fmt == "jpeg":
        if dtype != "uint8":
            raise ValueError(f"config.output.format jpeg holds 8-bit samples: output.dtype {dtype!r} contradicts it")
        if not 1 <= int(sec.get("quality", 90)) <= 100:
            raise ValueError(f"config.output.quality {sec.get('quality')!r}: 1 .. 100")
        if sec.get("restart_mcus", None) is not None and not 1 <= int(sec.get("restart_mcus")) <= 65535:
            raise ValueError(f"config.output.restart_mcus {sec.get('restart_mcus')!r}: 1 .. 65535")
        subsampling = jpeg_option("subsampling", sec.get("subsampling", "444"))
        huffman = jpeg_option("huffman", sec.get("huffman", "standard"))
        if subsampling == "420" and config.mode == "grey":
            raise ValueError("config.output.subsampling 420 needs three components: mode grey writes one")
        return OutputOptions(fmt, dtype, sec.get("quality", 90), sec.get("restart_mcus", None), subsampling, huffman)
    if fmt == "png":
        if dtype == "float32":
            raise ValueError("config.output.format png holds 8- or 16-bit samples: output.dtype 'float32' contradicts it")
        return OutputOptions(fmt, dtype, filter=png_option("filter", sec.get("filter", "adaptive")),
                             interval_bytes=png_option("interval_bytes", sec.get("interval_bytes", None)))
    return OutputOptions(fmt, dtype)


def _plain(value):
    """A list node of the configuration as a plain list (scalars and None pass)."""
    return list(value) if hasattr(value, "__len__") and not isinstance(value, (str, bytes)) else value


def intake_options(burst_path, config):
    """reference_options, noise_profile.noise_options and white_balance.wb_options as an IntakeOptions, checked in that
    order, plus the refusals of ``white_balance.source: estimate`` that need no burst — ``mode: grey`` and a folder of .dng
    files, which comes back normalised: each a ValueError before the burst is touched or anything is uploaded."""
    intake = IntakeOptions(reference_options(config)[0], *noise_options(config), *wb_options(config))
    if intake.wb_source == "estimate":
        if config.mode == "grey":
            raise ValueError("config.white_balance.source 'estimate' with mode grey: a monochrome sensor has no white balance")
        if isinstance(burst_path, (str, os.PathLike)) and not str(burst_path).endswith(".npz"):
            raise ValueError("config.white_balance.source 'estimate' needs integer sensor counts: a folder of .dng files "
                             "comes back normalised and balanced by its own AsShotNeutral")
    return intake


DNG_READERS = ("rawpy", "native")


def dng_options(config):
    """The reader of a folder of .dng files: the optional section config.dng = {"reader": "rawpy" | "native"} (not in the
    reference schema, like config.output; absent: "rawpy").  ValueError for anything else."""
    reader = str((config.get("dng", None) or {}).get("reader", "rawpy"))
    if reader not in DNG_READERS:
        raise ValueError(f"config.dng.reader {reader!r}: rawpy or native")
    return reader


DNG_LINEARIZATION = ("refuse", "apply")


def dng_linearization(config):
    """What the native reader does with a file's LinearizationTable, BlackLevelDeltaH / V and GainMap opcodes:
    config.dng.linearization = "refuse" (absent: the table and non-zero deltas are a ValueError, the maps are ignored) or
    "apply" (dng.read_dng_burst(linearization=True): read and applied on the GPU).  ValueError for anything else, and for
    "apply" with the rawpy reader, which has no such step."""
    choice = str((config.get("dng", None) or {}).get("linearization", "refuse"))
    if choice not in DNG_LINEARIZATION:
        raise ValueError(f"config.dng.linearization {choice!r}: refuse or apply")
    if choice == "apply" and dng_options(config) != "native":
        raise ValueError("config.dng.linearization 'apply' needs config.dng.reader 'native': the rawpy reader applies none of it")
    return choice


def load_burst(burst_path, config):
    """The burst mapping of process(): `burst_path` itself, the arrays of an .npz file, or a folder of .dng files, which
    needs rawpy + exifread like the reference (absent from this image: ImportError) and takes the noise profile, ISO,
    orientation and colour matrix from the tags of file 0 — or, with ``config.dng.reader: native`` (dng_options, checked
    before the burst is touched), is read by dng.read_dng_burst with the standard library and the GPU alone; a file without
    NoiseProfile then needs ``noise_model.source: estimate``.  ``config.dng.linearization: apply`` (dng_linearization,
    checked there too) has that reader apply the files' linearization table, black deltas and gain maps.  ``mode: grey``:
    ``cfa_pattern`` / ``white_balance`` are filled in."""
    reader = dng_options(config)
    linearization = dng_linearization(config) == "apply"
    burst = burst_path
    if isinstance(burst_path, (str, os.PathLike)) and str(burst_path).endswith(".npz"):
        burst = dict(np.load(burst_path))
    elif isinstance(burst_path, (str, os.PathLike)) and reader == "native":
        from .dng import read_dng_burst

        burst = read_dng_burst(burst_path, mode=config.mode, linearization=linearization)
        if "alpha" not in burst and noise_options(config)[0] != "estimate" and config.noise_model.get("alpha", None) is None:
            raise ValueError(f"{burst['debug']['infos'][0].path}: NoiseProfile (50761) is missing: set "
                             "noise_model.source: estimate to measure the noise profile from the frames")
    elif isinstance(burst_path, (str, os.PathLike)):
        ref_raw, raw_comp, iso, tags, cfa, _, white_balance, _ = load_dng_burst(burst_path)  # needs rawpy + exifread
        nm = tags["Image Tag 0xC761"].values  # DNG NoiseProfile, already scaled for the ISO (reference :232-238)
        if config.mode == "grey":  # one (alpha, beta) pair (reference :233-235)
            alpha_beta = {"alpha": nm[0][0], "beta": nm[1][0]}
        else:                      # mean over the three colour planes (reference :236-238)
            alpha_beta = {"alpha": sum(x[0] for x in nm[::2]) / 3, "beta": sum(x[0] for x in nm[1::2]) / 3}
        burst = {"ref": ref_raw, "comp": raw_comp, "iso": iso, "cfa_pattern": cfa, "white_balance": white_balance,
                 **alpha_beta}
        if "Image Orientation" in tags:
            burst["orientation"] = tags["Image Orientation"].values[0]
        if "Image Tag 0xC621" in tags:  # DNG ColorMatrix1 (raw2rgb.py:12-27)
            burst["xyz2cam"] = np.array([x.decimal() for x in tags["Image Tag 0xC621"].values], np.float32).reshape(3, 3)
    if config.mode == "grey":  # monochrome sensor: no colour filter array, no white balance (both unused by main())
        burst = dict(burst)
        burst.setdefault("cfa_pattern", [[0, 1], [1, 2]])
        burst.setdefault("white_balance", [1.0, 1.0, 1.0])
    return burst


def merge_stage(burst, intake, config):
    """From the burst mapping to main(): (merged image, debug_dict, number of comparison frames), in this order.
    ``reference.select: sharpest`` (absent or "first": ``ref`` is the base frame, as in the reference, which takes file 0 —
    nothing of this step runs then): the first ``candidates`` frames of the burst (clamped to its length) are scored on the
    GPU in the form they come in (select_reference, hhsr_frame_sharpness), the sharpest becomes ``ref`` and the others keep
    their order as ``comp``; everything derived from the reference frame — its brightness and the SNR-based parameters, the
    early normalisation of an integer burst — follows the chosen frame.  ``debug_dict["reference index"]`` is its position in
    the original burst, ``debug_dict["sharpness"]`` the candidates' scores (float64 ndarray).  The candidates are uploaded
    once for the score and again by main().  For a folder of .dng files the frame arrays are reordered; the tags (noise
    profile, ISO, orientation, colour matrix) stay those of file 0.
    ``white_balance.source: estimate`` (absent or "given": the burst's ``white_balance``, and nothing of this step runs): a
    Bayer burst of integer counts needs no ``white_balance`` key — the gains are measured on the GPU
    (white_balance.estimate_white_balance: hhsr_white_balance_hist, hhsr_white_balance_fit) from the reference frame's
    counts, after the reference selection and before anything is normalised, with ``frames`` > 1 from the next frames' counts
    as well (clamped to the burst's length).  The burst's own ``white_balance`` is ignored; the estimate is what the
    normalisation of every frame, the noise estimate and prepare_config() / ``config.exif`` see, and ``debug_dict["white
    balance"]`` is the estimator's dict (white_balance, tiles, tiles_gated).  It is a grey-world estimate: a scene whose
    balanced channel means differ is estimated wrong by that difference.  Frames that are not integer counts (float frames
    are already balanced) are a ValueError before anything is uploaded; fewer than ``min_tiles`` usable tiles is the
    ValueError of fit_white_balance.
    Integer frames (raw_frames.RawLayout.from_burst) are sensor counts + metadata: the normalisation / white balance of
    utils_dng.py:149-160, on the GPU.  The reference frame now (its brightness picks the SNR-based parameters); the other
    frames stay integer host arrays and are uploaded as counts or packed rows — half the bytes of float32 frames or less —
    and normalised frame by frame on the pipeline streams (BurstPipeline._ingest, told by ``config.hip.raw_norm``),
    overlapping the other frames' kernels.
    ``noise_model.source: estimate`` (absent or "given": the burst's ``alpha`` / ``beta``), with ``noise_model.frames``
    (default 1) and ``noise_model.min_tiles`` (default 16): the noise profile is measured on the GPU
    (noise_profile.estimate_noise_profile: hhsr_noise_profile_hist, hhsr_noise_profile_fit) from the normalised reference
    frame — after the reference selection — and with ``frames`` > 1 from the next frames as well (clamped to the burst's
    length); the burst's own ``alpha`` / ``beta`` are ignored, the estimate feeds the curve estimators and prepare_config()
    like a given pair (``config.noise_model.alpha`` / ``.beta`` hold it afterwards — so a configuration object that went
    through an estimating call is reset (alpha: None) before the next, or noise_options refuses it) and ``debug_dict["noise
    profile"]`` is the estimator's dict (alpha, beta, per_colour, bins_used).  On a textured scene the estimate is an upper
    bound (noise_profile.py).
    Noise curves: given in the burst, or ``config.noise_model.estimator``: "monte_carlo" (default — the reference's estimator
    run_fast_MC, super_resolution.py:252, whose curves include the clipping of the noisy samples to [0, 1]: near black and
    near saturation sigma_t and d_t are up to ~1.6x smaller than the un-clipped law; seeded by
    ``config.noise_model.seed``, default 0, so process() is reproducible where the reference is not, D18), "monte_carlo_hip"
    (the same estimator as one fused kernel of the C library, hhsr_noise_mc: its own seeded stream, stated in include/hhsr.h,
    so its curves differ from "monte_carlo" by Monte-Carlo noise) or "analytic" (the un-clipped limit, synthetic.noise_curves
    — what prepare_config() uses when called directly)."""
    ref_raw, raw_comp = burst["ref"], burst["comp"]
    layout = RawLayout.from_burst(burst, ref_raw)
    if intake.wb_source == "estimate" and not layout.is_counts:
        raise ValueError("config.white_balance.source 'estimate' needs integer sensor counts (with black_levels and "
                         "white_level): float frames are taken as normalised and already white-balanced")
    debug = {}
    if intake.ref_select == "sharpest":  # the chosen frame is `ref` from here on
        index, scores = select_reference(ref_raw, raw_comp, config, burst["cfa_pattern"], layout)
        ref_raw, raw_comp = reorder_burst(ref_raw, raw_comp, index)
        debug.update({"reference index": int(index), "sharpness": np.asarray(scores, np.float64)})
    if intake.wb_source == "estimate":  # the burst's own white_balance is ignored
        wb_estimate = estimate_burst_white_balance(ref_raw, raw_comp, burst, layout, intake.wb_frames, intake.wb_min_tiles)
        burst = dict(burst, white_balance=wb_estimate["white_balance"])
    if layout.is_counts:
        ref_raw = layout.normalize(np.asarray(ref_raw), burst["white_balance"], burst["cfa_pattern"])
        raw_comp = [np.asarray(f) for f in raw_comp]
        config.hip = dict(getattr(config, "hip", None) or {}, raw_norm=layout.raw_norm())  # (a fresh mapping: the caller's is not edited)
        ref_for_stats = np.full((1, 1), ref_raw.mean().item(), np.float32)
    else:
        ref_raw = np.asarray(ref_raw, dtype=np.float32) if not torch.is_tensor(ref_raw) else ref_raw
        raw_comp = np.asarray(raw_comp, dtype=np.float32) if not torch.is_tensor(raw_comp) else raw_comp
        ref_for_stats = ref_raw
    std_curve, diff_curve = burst.get("std_curve"), burst.get("diff_curve")
    alpha, beta = burst.get("alpha"), burst.get("beta")
    if intake.noise_source == "estimate":  # the burst's own alpha / beta are ignored
        debug["noise profile"] = estimate_burst_profile(ref_raw, raw_comp, burst, layout, config, intake.noise_frames,
                                                        intake.noise_min_tiles)
        alpha, beta = debug["noise profile"]["alpha"], debug["noise profile"]["beta"]
    if intake.wb_source == "estimate":
        debug["white balance"] = wb_estimate
    estimator = config.noise_model.get("estimator", "monte_carlo")
    if (std_curve is None or diff_curve is None) and estimator in ("monte_carlo", "monte_carlo_hip"):
        from .fast_monte_carlo import run_fast_MC  # the reference's estimator (super_resolution.py:252), seeded

        if config.noise_model.get("alpha", None) is not None:
            alpha, beta = config.noise_model.alpha, config.noise_model.beta
        std_curve, diff_curve = run_fast_MC(float(alpha), float(beta), seed=int(config.noise_model.get("seed", 0)),
                                            engine="hip" if estimator == "monte_carlo_hip" else "torch")
    prepare_config(config, ref_for_stats, alpha, beta, burst["cfa_pattern"], burst["white_balance"],
                   int(burst.get("iso", 100)), std_curve, diff_curve, shape=tuple(ref_raw.shape))
    out, debug_dict = main(ref_raw, raw_comp, config)
    debug_dict.update(debug)
    return out, debug_dict, len(raw_comp)


def finish(out, debug_dict, burst, n_comp, output, config):
    """After main() (reference super_resolution.py:303-356), all on the GPU (utils_image.py, raw2rgb.py; only the finished
    image is copied to the host): the frame-count denoisers (``accumulated_robustness_denoiser.median / .gauss``), then
    ``postprocessing`` (colour matrix, unsharp mask, devignetting, gamma — ON by default like the reference's YAML; tone
    mapping is the device implementation of the algorithm include/hhsr.h restates, never compared with an OpenCV run:
    raw2rgb.postprocess with restated_tonemapping=True) and the EXIF orientation, then what `output` (output_options) asks
    for.  With an integer dtype and ``robustness.save_mask``, ``debug_dict["robustness mask"]`` is the reference's mask
    image: uint8 [sH, sW], accumulated robustness / number of comparison frames, nearest neighbour (hhsr_encode_mask); it
    stays that uint8 array with ``format: jpeg``, ``png`` and ``dng``.  ``format: dng`` keeps the linear image: the
    denoisers run, post-processing is off (output_options) and the image is NOT rotated — the orientation becomes the file's
    Orientation tag; the mask and ``debug_dict["accumulated robustness"]`` are oriented as for the other formats."""
    den = config.accumulated_robustness_denoiser
    half_index = bool((config.get("compat", None) or {}).get("post_denoiser_half_index", True))
    for stage, denoise in ((den.median, frame_count_denoising_median), (den.gauss, frame_count_denoising_gauss)):
        if stage.enabled:
            out = denoise(out, debug_dict["accumulated robustness"], stage, scale=config.scale, half_index=half_index,
                          mode=config.mode)
    ori = int(burst.get("orientation", 1))  # EXIF 'Image Orientation' (reference :346-352)
    pp = config.postprocessing
    dng = output.format == "dng"  # the linear image as it was merged: the orientation goes into the file's tag
    if pp.enabled and not dng:
        out = raw2rgb.postprocess(burst.get("rawpy_image", None), out, pp.do_color_correction, pp.do_tonemapping,
                                  pp.do_gamma_correction, pp.sharpening, pp.do_devignetting, burst.get("xyz2cam", None),
                                  orientation=ori, restated_tonemapping=True)
    elif not dng:
        out = apply_orientation(out, ori)
    acc_oriented = apply_orientation(debug_dict["accumulated robustness"], ori) if "accumulated robustness" in debug_dict else None
    channels = 1 if config.mode == "grey" else None
    if output.dtype == "float32":
        output_image = out.cpu().numpy()
    elif output.format == "jpeg":  # the whole file's bytes, coded on the device: a tenth of the uint8 samples cross the link
        output_image = encode_jpeg(out, quality=output.quality, restart_mcus=output.restart_mcus, channels=channels,
                                   subsampling=output.subsampling, huffman=output.huffman)
    elif output.format == "png":  # the whole file's bytes again: filtered and deflate-coded on the device
        output_image = encode_png(out, bits=16 if output.dtype == "uint16" else 8, channels=channels, filter=output.filter,
                                  interval_bytes=output.interval_bytes)
    elif dng:  # a LinearRaw DNG: lossless-JPEG tiles coded on the device, the file's bytes cross the link
        wb = burst.get("white_balance", None)
        output_image = encode_dng(out, channels=channels, tile=output.tile, predictor=output.predictor,
                                  xyz2cam=burst.get("xyz2cam", None), white_balance=None if wb is None else np.asarray(wb),
                                  orientation=ori, camera_model=burst.get("camera_model", None),
                                  calibration_illuminant=burst.get("calibration_illuminant", None))
    else:  # integer output: encoded on the device, 3 or 6 instead of 12 bytes per pixel cross the host link
        output_image = encode_image(out, output.dtype, channels=channels).cpu().numpy()
    if output.dtype != "float32" and acc_oriented is not None and config.robustness.save_mask:  # the reference's `.rob.png`
        mask_shape = tuple(out.shape[:2])[::-1] if dng and ori >= 5 else tuple(out.shape[:2])  # (the mask is oriented)
        debug_dict["robustness mask"] = robustness_mask(acc_oriented, max(1, n_comp),  # (no comparison frame: the map is 0)
                                                        mask_shape).cpu().numpy()
    if acc_oriented is not None:
        debug_dict["accumulated robustness"] = acc_oriented.cpu().numpy()
    return output_image, debug_dict


def process(burst_path, config):
    """process(burst_path, config) -> (float32 ndarray [sH, sW, 3], debug_dict)   (reference :203-360).

    `burst_path` is either a burst held in memory / in an .npz file — a mapping with keys ``ref`` [H,W], ``comp`` [N-1,H,W],
    ``cfa_pattern`` [2,2], ``white_balance`` [>=3], ``alpha``, ``beta`` and optionally ``iso``, ``std_curve``,
    ``diff_curve``, ``orientation`` (EXIF 1..8), ``xyz2cam`` (3x3, DNG ColorMatrix1, for
    ``postprocessing.do_color_correction``) — ``cfa_pattern`` / ``white_balance`` may be left out with ``mode: grey``
    (monochrome sensors: channel 0 of the result is the image, channels 1 and 2 are NaN like the reference's); ref / comp are
    either normalised white-balanced float RAW or integer sensor counts with ``black_levels`` and ``white_level`` (normalised
    on the GPU like utils_dng.py:149-160), either uint16 or, with ``packing`` (a name of utils_dng.PACKINGS) and ``width``
    (may be left out when the rows hold no padding), the packed 10/12/14-bit rows as uint8 [H, row_bytes] — or a folder of
    .dng files (load_burst).  The optional sections are checked in this order before the burst is touched and documented
    where they act: ``config.output`` (output_options, finish), then ``config.reference``, ``config.noise_model`` (source,
    frames, min_tiles; estimator, seed) and ``config.white_balance`` (intake_options, merge_stage); the denoisers,
    ``postprocessing`` and the orientation: finish."""
    output = output_options(config)
    intake = intake_options(burst_path, config)
    burst = load_burst(burst_path, config)
    out, debug_dict, n_comp = merge_stage(burst, intake, config)
    return finish(out, debug_dict, burst, n_comp, output, config)

