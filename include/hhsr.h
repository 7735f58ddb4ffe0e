/*
 * hhsr.h — C ABI of libhhsr_hip.so: the MI355X (gfx950) kernels of the handheld burst
 * super-resolution hot path.
 *
 * The reference (Jamy-L/Handheld-Multi-Frame-Super-Resolution) has no native layer: its hot path
 * is 25 Numba-CUDA kernels plus torch ops launched from Python.  Each entry point below replaces
 * one of those launch sites (cited as file:line relative to the reference's
 * handheld_super_resolution/ package).  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller unless the parameter is documented as
 *    "host"; functions never allocate, free or synchronise (the hhsr_grey_plan_create/destroy pair
 *    excepted): they only enqueue work on `stream` (a hipStream_t passed as void*; NULL = null stream);
 *  - images are row-major float32; `pitch` arguments are in ELEMENTS: the distance between the starts of two rows,
 *    >= the width (error -1 otherwise).  A pitch lets a caller pass a hipMallocPitch buffer or a window of a larger
 *    frame without a copy: nothing between the end of a row and the start of the next is read into a result or
 *    written.  Only the arguments that have a pitch can be padded: flows, Hessians, covariances, robustness maps,
 *    guide statistics and every output of the merge are COMPACT whatever the raw pitch is.  Pointers need the
 *    alignment of their element type unless an entry point says more;
 *  - flow fields are float32 [ny][nx][2] = (dx, dy) per tile, moving(p + flow) ~ ref(p);
 *  - covariances are float32 [H/2][W/2][2][2]; accumulators float32 [sH][sW][3];
 *  - the CFA is 4 bytes {c00, c01, c10, c11} with 0=R, 1=G, 2=B;
 *  - return value: 0 = OK, >0 = hipError_t of the launch, <0 = invalid argument; the message is
 *    available from hhsr_last_error() (thread local).  No C++ exception crosses the boundary.
 *  - no global mutable state: re-entrant across host threads and streams (a grey plan is caller-owned
 *    state).
 */
#ifndef HHSR_H
#define HHSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HHSR_VERSION_MAJOR 0
#define HHSR_VERSION_MINOR 1

#define HHSR_MAX_TAPS 33      /* Gaussian taps: 4*factor+1, factor <= 8 */
#define HHSR_MAX_FRAMES 64    /* frames per hhsr_merge_burst launch */
#define HHSR_MAX_BATCH 8      /* frames per launch of the batched front-end entry points (hhsr_*_batch) */
#define HHSR_MAX_EXPOSURES 4  /* exposures per hhsr_post_expose / hhsr_mertens call */

const char* hhsr_version(void);
const char* hhsr_last_error(void);

/* ---- grey image: mask of the ideal half-band low-pass (utils_image.py:82-100) -----------------
 * The reference zeroes the outer quarter bands of the fftshift-ed full complex spectrum and keeps
 * the real part of the inverse.  hhsr_lowpass_mask_c2c zeroes the same bins of an UN-shifted
 * complex64 spectrum [H][W] in place.  hhsr_lowpass_mask_r2c applies the equivalent Hermitian
 * mask m'(k) = (m(k) + m(-k))/2 in {0, 1/2, 1} to a half spectrum [H][W/2+1] (rfft2 layout), so
 * that irfft2 returns exactly Re(ifft2(mask * fft2(x))). `spec` = interleaved (re, im) float32.
 * stride_y / stride_x: element (complex) strides of the two spectrum dimensions — rocFFT hands torch a
 * transposed half spectrum, which is masked in place as it lies. */
int hhsr_lowpass_mask_c2c(float* spec, int H, int W, int64_t stride_y, int64_t stride_x, void* stream);
int hhsr_lowpass_mask_r2c(float* spec, int H, int W, int64_t stride_y, int64_t stride_x, void* stream);

/* Planned grey transform: real-to-complex rocFFT plan -> Hermitian low-pass mask (normalisation folded
 * in) -> complex-to-real plan; dst = Re(ifft2(mask * fft2(src))), src/dst contiguous [H][W], src intact.
 * hhsr_grey_plan_create is the ONE place the library allocates (the plan and its [H][W/2+1] spectrum
 * buffer, owned by the plan); a plan is mutable state: use it from one stream at a time.
 * Returns 1000 + hipfftResult on a hipFFT error. */
#define HHSR_GREY_PRUNED 1   /* batched row plans + strided column plans on the kept x-bins only (experiment) */
#define HHSR_GREY_FUSED 4    /* three in-LDS kernels (rows, columns + mask, rows) when W is even, W/2 and H have no prime
                                factor above 19 and their transforms fit the kernels' LDS and thread budgets
                                (hhsr_grey_plan_query tells); otherwise the library plans are used */
#define HHSR_GREY_TPRUNED 2  /* row plans with a transposed spectrum + contiguous column plans on the kept bins */
#define HHSR_GREY_BATCH(n) ((n) << 8)  /* the plan holds n (<= HHSR_MAX_BATCH) spectra: hhsr_grey_lowpass_batch then
                                          transforms n frames with ONE launch per phase (default 1) */
int hhsr_grey_plan_create(int H, int W, int flags, void** plan_out);
int hhsr_grey_lowpass(void* plan, const float* src, float* dst, void* stream);
/* The same transform for n_frames frames (HOST arrays of device pointers): per-frame results are bit-identical to
 * hhsr_grey_lowpass; with the fused kernels the row blocks / kept columns of all frames of a plan-batch share one
 * launch per phase (the per-frame launches are latency-bound: 3 x 19 launches of ~40 us per 12 MP burst). */
int hhsr_grey_lowpass_batch(void* plan, const float* const* srcs, float* const* dsts, int n_frames, void* stream);
int hhsr_grey_plan_destroy(void* plan);
/* Which route a plan takes.  out (HOST, n >= HHSR_GREY_INFO_LEN values; the unused ones are 0):
 *   [0] 1 = the fused kernels run, 0 = the library plans (every other value is 0 then)
 *   [1] rows per workgroup and [2] threads per workgroup of the row kernels, [3] kept columns per workgroup
 *   [4] / [5] id of the compile-time plan of the row / column kernels (0: run-time passes)
 *   [6] / [7] LDS bytes per workgroup of the row / column kernels, [8] kept x-bins
 *   [9] / [10] number of passes of the W/2-point / H-point transforms
 *   [16 .. 32) the radices of the W/2-point passes, [32 .. 48) those of the H-point passes, in execution order.
 * hhsr_grey_plan_query answers for the plan that hhsr_grey_plan_create(H, W, flags, .) WOULD build and makes no HIP
 * call (usable without a device); hhsr_grey_plan_info reports a live plan.
 * hhsr_grey_radix_schedule: the schedule of `seqs` simultaneous n_points-point transforms in a workgroup of `threads`
 * threads, as the kernels' host side searches it: out[0] = number of passes (0: no schedule), out[1 ..] the radices
 * (HOST, n >= 1 + 16 values).  No HIP call. */
#define HHSR_GREY_INFO_LEN 48
int hhsr_grey_plan_query(int H, int W, int flags, int32_t* out, int n);
int hhsr_grey_plan_info(void* plan, int32_t* out, int n);
int hhsr_grey_radix_schedule(int n_points, int seqs, int threads, int32_t* out, int n);

/* ---- pyramid (alignment.py:27-37, 74-82; utils_image.py:360-391) ------------------------------ */
/* dst[y][x] = src[y mod H][x mod W], dst is Hp x Wp (F.pad 'circular', bottom/right); src_pitch >= W, dst_pitch >= Wp,
 * the padding columns of dst are left as they are. */
int hhsr_pad_circular(const float* src, int H, int W, int src_pitch,
                      float* dst, int Hp, int Wp, int dst_pitch, void* stream);
/* Valid separable Gaussian (rows then columns) + decimation by `factor`:
 * dst is floor((H-2r)/f) x floor((W-2r)/f), r = (ntaps-1)/2; factor 2 or 4 with ntaps = 4*factor+1 (the reference's kernels).  `taps` is a HOST array.
 * src_pitch >= W, dst_pitch >= the output width; the padding columns of dst are left as they are. */
int hhsr_gauss_decimate(const float* src, int H, int W, int src_pitch,
                        float* dst, int dst_pitch, int factor,
                        const float* taps, int ntaps, void* stream);
/* n_frames levels of the same shape in one launch (HOST arrays of device pointers; one src_pitch and one dst_pitch for all
 * of them); per frame bit-identical. */
int hhsr_gauss_decimate_batch(const float* const* srcs, int n_frames, int H, int W, int src_pitch,
                              float* const* dsts, int dst_pitch, int factor,
                              const float* taps, int ntaps, void* stream);

/* ---- Lucas-Kanade precompute (ICA.py:15-76) ---------------------------------------------------
 * gx = I[x+1]-I[x-1], gy likewise (zero border, no 1/2 factor); hess[ty][tx] = sum over the tile of
 * [gx^2, gx gy; gx gy, gy^2] for the floor(H/ts) x floor(W/ts) tile grid.
 * gx and gy are written AT THE INPUT'S PITCH (each needs H * pitch elements; their padding columns are left as they are) —
 * the layout hhsr_ica reads them in; hess is compact. */
int hhsr_grad_hessian(const float* lvl, int H, int W, int pitch, int ts,
                      float* gx, float* gy, float* hess, void* stream);

/* ---- block matching (block_matching.py:20-76, 348-377 and 78-345) -----------------------------
 * L2: argmin over (2r+1)^2 integer shifts of the tile SSD (== the reference's
 * sum(win^2) - 2 corr(ref, win) up to a per-tile constant), window origin
 * tile*ts + round_half_even(flow) - r with clamp-to-edge addressing of the moving level, first
 * minimum in row-major order; the shift is ADDED to the un-rounded flow.
 * L1 (mode 0): the INTENDED semantics of the reference's undefined-behaviour kernels — SAD, zero
 * outside the moving level, flow <- round(flow) + shift.  mode 1: flow <- round_half_even(flow).
 * The reference level is ny*ts x nx*ts: ref_pitch >= nx * ts, mov_pitch >= mw (error -1 otherwise); the two pitches are
 * independent of each other. */
int hhsr_bm_l2(const float* ref, int ref_pitch, const float* mov, int mh, int mw, int mov_pitch,
               float* flow, int ny, int nx, int ts, int r, void* stream);
int hhsr_bm_l1(const float* ref, int ref_pitch, const float* mov, int mh, int mw, int mov_pitch,
               float* flow, int ny, int nx, int ts, int r, int mode, void* stream);

/* ---- ICA (ICA.py:78-482): n_iter Gauss-Newton steps per tile, in place on `flow`.
 * flags bit 0: reproduce the ts=64 row off-by-one of ica_kernel_64 (ICA.py:437-449).
 * ref, gx and gy share ONE layout, ref_pitch (>= nx * ts): pass gx / gy as hhsr_grad_hessian wrote them for `ref` at that
 * pitch; mov_pitch >= mw. */
int hhsr_ica(const float* ref, const float* gx, const float* gy, int ref_pitch, const float* hess,
             const float* mov, int mh, int mw, int mov_pitch,
             float* flow, int ny, int nx, int ts, int n_iter, int flags, void* stream);

/* ---- one pyramid level in one launch: block matching then ICA (alignment.py:125-147), ts in {8, 16, 32}.
 * metric: 0 = L2, 1 = L1 (intended semantics), 2 = L1_ref_effective.  Gradients are taken from the
 * reference level itself (rh x rw) — bit-identical to hhsr_grad_hessian's — `hess` from hhsr_grad_hessian.
 * Same results as hhsr_bm_* followed by hhsr_ica (flags bit 0 is irrelevant below ts = 64).
 * Incoming flow: `flow` itself (coarse_flow NULL, rep >= 0); or the nearest-neighbour upscaling of the coarser
 * level fused in (alignment.py:150-172): mult * coarse_flow[ty/rep][tx/rep] ([cny][cnx][2], zero past it); or
 * zero (coarse_flow NULL, rep < 0: the coarsest level).  `flow` is always the output.
 * ref_pitch >= rw, mov_pitch >= mw (error -1 otherwise), independent of each other; hess and the flows are compact. */
int hhsr_align_level(const float* ref, int rh, int rw, int ref_pitch, const float* hess,
                     const float* mov, int mh, int mw, int mov_pitch,
                     float* flow, int ny, int nx, int ts, int r, int metric, int n_iter,
                     const float* coarse_flow, int cny, int cnx, int rep, float mult, void* stream);
/* The same level step for n_frames moving frames against ONE reference level in one launch (HOST arrays of device
 * pointers; coarse_flows NULL or one pointer per frame): the coarse levels are 7-27 us launches of a few hundred
 * workgroups each — a chunk of frames fills the GPU where one frame cannot.  Per frame bit-identical.  One mov_pitch for
 * all moving levels. */
int hhsr_align_level_batch(const float* ref, int rh, int rw, int ref_pitch, const float* hess,
                           const float* const* movs, int n_frames, int mh, int mw, int mov_pitch,
                           float* const* flows, int ny, int nx, int ts, int r, int metric, int n_iter,
                           const float* const* coarse_flows, int cny, int cnx, int rep, float mult, void* stream);

/* ---- flow upscaling, nearest mode (alignment.py:150-172): dst[y][x] = mult*src[y/rep][x/rep],
 * zero where y/rep >= sny or x/rep >= snx. */
int hhsr_flow_upscale_nearest(const float* src, int sny, int snx, float* dst, int dny, int dnx,
                              int rep, float mult, void* stream);

/* ---- kernel covariances, Alg. 5 (kernels.py:29-243; utils_image.py:117-170, 346-357;
 * linalg.py:87-185), bayer mode: GAT -> 2x2 mean -> gradients -> structure tensor -> eigen ->
 * (k1, k2) -> covariance per Bayer quad.  law: 0 = hard_threshold, 1 = linear.
 * The four Bayer passes over a raw frame (hhsr_cov_from_raw, hhsr_rob_stats, hhsr_frame_stats, hhsr_frame_stats_batch) load
 * the (even, odd) pixel pair of a quad row at once: `pitch` must be EVEN and `raw` 8-byte aligned — a window of a larger
 * frame starts at an even column — and covs 16-byte aligned (error -1 otherwise).  An odd last row / column belongs to no
 * quad and is not read.  means / vars / covs are compact. */
int hhsr_cov_from_raw(const float* raw, int H, int W, int pitch, float* covs,
                      double alpha, double beta, double k_detail, double k_denoise,
                      double D_th, double D_tr, double k_stretch, double k_shrink, int law,
                      void* stream);

/* ---- robustness, Alg. 6-9 (robustness.py) -----------------------------------------------------*/
/* Guide image + 3x3 local mean / variance at guide resolution [3][H/2][W/2]
 * (robustness.py:207-225, 269-294).  wb: HOST double[3].  vars may be NULL (comp frames only need the means). */
int hhsr_rob_stats(const float* raw, int H, int W, int pitch, const uint8_t cfa[4],
                   const double* wb, float* means, float* vars, void* stream);
/* hhsr_rob_stats + hhsr_cov_from_raw in one pass over the raw frame (both work on the same Bayer-quad tile):
 * what super_resolution.py:137-163 computes per frame from the raw image alone.  vars may be NULL. */
int hhsr_frame_stats(const float* raw, int H, int W, int pitch, const uint8_t cfa[4], const double* wb,
                     float* means, float* vars, float* covs, double alpha, double beta, double k_detail,
                     double k_denoise, double D_th, double D_tr, double k_stretch, double k_shrink, int law,
                     void* stream);
/* The same pass for n_frames comp frames (guide means + covariances, no variances) in one launch: HOST arrays of
 * device pointers; one (even) pitch for all frames, every raws[n] 8-byte aligned; per frame bit-identical to
 * hhsr_frame_stats. */
int hhsr_frame_stats_batch(const float* const* raws, int n_frames, int H, int W, int pitch, const uint8_t cfa[4],
                           const double* wb, float* const* means, float* const* covs, double alpha, double beta,
                           double k_detail, double k_denoise, double D_th, double D_tr, double k_stretch,
                           double k_shrink, int law, void* stream);
/* Dodgson-quadratic x2 upsampling of a [3][lh][lw] map to [3][2lh][2lw], optionally warped by the
 * per-tile flow (NULL = reference frame; robustness.py:359-421).  +inf outside. */
int hhsr_rob_upscale(const float* stats, int lh, int lw, const float* flow, int ny, int nx, int ts,
                     float* out, void* stream);
/* Per-tile flow-irregularity map S (robustness.py:570-612): spread of the flow over the 3 x 3 TILE neighbourhood.
 * rows_before / rows_after (0 for a whole field): tile rows that lie in memory before flow[0] / after flow[ny - 1] —
 * `flow` is then a row slice of a larger field (the row slabs of the multi-GPU path, distributed.py) and the
 * neighbourhood reads them, so that the first and last rows of the slice get the weights of the full field. */
int hhsr_rob_s(const float* flow, int ny, int nx, double Mt, float s1, float s2, float* S, int rows_before,
               int rows_after, void* stream);
/* Frame-independent noise-model terms (robustness.py:505-528, once per burst):
 * sigma_sq[p] = sum_c max(ref_vars[c][p], std_curve[round(1000 ref_means[c][p])]^2), float32 [H][W];
 * curve_index[p] (optional, NULL to skip; needs ncurve <= 1024) = the three curve indices
 * round(1000 ref_means[c][p]) packed 10 bits each (c = 0 in the low bits), uint32 [H][W]. */
int hhsr_rob_sigma(const float* ref_means, const float* ref_vars, int H, int W,
                   const double* std_curve, int ncurve, float* sigma_sq, uint32_t* curve_index, void* stream);
/* hhsr_rob_upscale(means) + hhsr_rob_upscale(vars) + hhsr_rob_sigma in one pass over the reference frame's guide
 * statistics [3][lh][lw] (robustness.py:23-76 and 505-528, once per burst): ref_means float32 [3][2lh][2lw],
 * sigma_sq [2lh][2lw], curve_index (optional) — bit-identical to the three calls; the upsampled variances are
 * never written. */
int hhsr_ref_planes(const float* guide_means, const float* guide_vars, int lh, int lw,
                    const double* std_curve, int ncurve, float* ref_means, float* sigma_sq,
                    uint32_t* curve_index, void* stream);
/* Fused warp-upsample of the frame's guide means + colour distance + noise-model shrink + threshold
 * (robustness.py:359-421, 453-461, 505-528, 627-639) -> R float32 [2lh][2lw].
 * ref_sigma_sq / ref_curve_index from hhsr_rob_sigma; diff_curve: device double[ncurve].
 * Two kernels: with ts % 16 == 0, the packed curve indices and ncurve <= 1024 the fused float32 kernel of
 * hhsr_rob_frames with one frame (|dR| <= 1e-4 against the reference's float64 chain); otherwise (index plane NULL,
 * other tile sizes, longer curves) the slower generic kernel with the reference's float64 chain.  The fused kernel moves
 * 16-byte vectors where W % 4 == 0 and ref_means / ref_sigma_sq / ref_curve_index / R are 16-byte aligned and dwords
 * elsewhere: R does not depend on the alignment, bit for bit. */
int hhsr_rob_frame(const float* comp_means, int lh, int lw, const float* ref_means, const float* ref_sigma_sq,
                   const uint32_t* ref_curve_index, const float* flow, int ny, int nx, int ts, const float* S,
                   const double* diff_curve, int ncurve, double t, float* R, void* stream);
/* hhsr_rob_frame for n_frames frames of one burst (HOST arrays of device pointers): groups of 4 frames share one pass
 * over the reference-frame planes (20 of the 27 bytes per pixel and frame); per frame bit-identical to hhsr_rob_frame.
 * Where the fused kernel does not apply (see hhsr_rob_frame) the generic kernel runs once per frame.
 * S = NULL: the per-tile weights of hhsr_rob_s are evaluated inside the kernel from (Mt, s1, s2) — one launch less per
 * frame, the same bits as with the maps of hhsr_rob_s; only with the fused kernel (ts % 16 == 0, packed curve indices,
 * ncurve <= 1024; error -3 otherwise).  With S given, Mt / s1 / s2 are ignored.  flow_rows_before / flow_rows_after: as in hhsr_rob_s, for the
 * weights evaluated inside the kernel (every flows[n] is a row slice with that many tile rows around it). */
int hhsr_rob_frames(const float* const* comp_means, int n_frames, int lh, int lw, const float* ref_means,
                    const float* ref_sigma_sq, const uint32_t* ref_curve_index, const float* const* flows, int ny,
                    int nx, int ts, const float* const* S, double Mt, float s1, float s2, const double* diff_curve,
                    int ncurve, double t, float* const* R, int flow_rows_before, int flow_rows_after, void* stream);
/* 5x5 clamp-border minimum (robustness.py:670-686).  acc_r != NULL additionally does acc_r += r
 * (the accumulated robustness of super_resolution.py:158-159, fused to save a pass). */
int hhsr_local_min5(const float* R, int H, int W, float* r, float* acc_r, void* stream);
/* Accumulated robustness the way the reference keeps it where something DECIDES on it (super_resolution.py:116-117,
 * 158-159; utils.py:93-120; merge.py:223-228): the float64 sum of the n_frames (<= HHSR_MAX_FRAMES) maps rs[] (HOST array of
 * device pointers, float32 [H][W]) in frame order, in one pass.  load != 0: start from sum64 (bursts longer than one
 * call).  Outputs, each may be NULL (not all): sum64 double [H][W]; mask32 = the sum rounded to float32 (the map the API
 * reports); decisions32 = float32 map a with (a <= mfc) == (sum <= mfc) and (a < mfc) == (sum < mfc) for
 * mfc = max_frame_count — what hhsr_accumulate_ref compares as (double) a (exact for every mfc float32 can hold).
 * flags: HHSR_ROB_SUM_LOAD (= the former `load != 0`) | HHSR_ROB_SUM_MIN5: rs[] are the UN-filtered maps R and the sum is taken
 * over their 5 x 5 clamp-border minima (robustness.py:641-686; = hhsr_local_min5 per frame, then the sum) — for callers whose
 * merge applies the minimum itself (HHSR_MERGE_LOCAL_MIN) and never materialises the filtered maps. */
#define HHSR_ROB_SUM_LOAD 1
#define HHSR_ROB_SUM_MIN5 2
int hhsr_rob_sum(const float* const* rs, int n_frames, int H, int W, int flags, double max_frame_count, double* sum64,
                 float* mask32, float* decisions32, void* stream);

/* ---- monochrome sensors, `mode: grey` (super_resolution.py:106-109, 144-147; kernels.py:83-87; robustness.py:62-66,
 * 145-148, 337-343; merge.py:131-137, 191-194, 349-354, 410): the frame is its own grey image (alignment unchanged), its
 * own one-channel guide image (no white balance) and the kernel covariances are estimated per pixel.
 * hhsr_mono_frame_stats: 3x3 local mean / variance [H][W] and / or covariances [H][W][2][2] in one pass
 *   (means NULL: covariances only; covs NULL: statistics only; vars may be NULL); any pitch >= W, raw 4-byte aligned,
 *   covs 16-byte aligned; the outputs are compact.
 * hhsr_mono_rob_upscale: robustness.py:296-421 on a one-channel map, which keeps its size while the kernel keeps its
 *   hard-coded s = 2 — the top-left quadrant stretched over the frame (+inf outside), reproduced as it is;
 *   flow NULL = the reference frame.
 * hhsr_mono_rob_sigma / hhsr_mono_rob_frame: robustness.py:505-528 / the fused per-frame pass -> R, one channel.
 *   hhsr_mono_rob_frame: with W % 4 == 0, ts % 4 == 0 and 16-byte aligned ref_means / sigma_sq / R the float32
 *   4-pixels-per-thread kernel runs (|dR| <= 1e-4 like the fused Bayer kernel), otherwise the float64 one-pixel kernel. */
int hhsr_mono_frame_stats(const float* raw, int H, int W, int pitch, float* means, float* vars, float* covs,
                          double alpha, double beta, double k_detail, double k_denoise, double D_th, double D_tr,
                          double k_stretch, double k_shrink, int law, void* stream);
int hhsr_mono_rob_upscale(const float* stats, int H, int W, const float* flow, int ny, int nx, int ts, float* out,
                          void* stream);
int hhsr_mono_rob_sigma(const float* ref_means, const float* ref_vars, int H, int W, const double* std_curve,
                        int ncurve, float* sigma_sq, void* stream);
int hhsr_mono_rob_frame(const float* comp_means, int H, int W, const float* ref_means, const float* sigma_sq,
                        const float* flow, int ny, int nx, int ts, const float* S, const double* diff_curve,
                        int ncurve, double t, float* R, void* stream);

/* kflags of the merge entry points */
#define HHSR_KERNEL_ISO 1   /* merging.kernel == "iso": w = exp(-(dx^2+dy^2)) instead of the steerable kernel */
#define HHSR_WEIGHT_F64 2   /* evaluate covariance interpolation / weights in float64 like the reference's
                               Numba typing (validation mode; default = float32 weights, float64 geometry) */
/* hhsr_merge_burst only — restrict its kernel choice (validation, A/B measurements; default: fastest applicable): */
#define HHSR_MERGE_FORCE_GENERIC 4  /* no LDS staging: one thread per HR pixel, operands from global memory     */
#define HHSR_MERGE_FORCE_TILE 8     /* no x2 kernel: the 16 x 16 HR tile kernel                                  */
#define HHSR_MERGE_FORCE_X2V1 16    /* x2: first-generation kernel (per-pixel geometry) instead of k_merge_x2    */
/* hhsr_accumulate_ref only: */
#define HHSR_REF_DIVIDE 64   /* normalise in the same pass: num = (num (+) ref) / (den (+) ref), den is read and left as it is —
                                accumulate_ref followed by divide (super_resolution.py:187-190) without a second pass over
                                the accumulators; bit-identical to hhsr_accumulate_ref + hhsr_divide                    */
#define HHSR_REF_FAST 128    /* float32 weight chain for the pixels the accumulated-robustness rule leaves alone, outside the
                                border bands — what hhsr_merge_burst does for its reference frame; default: the reference's
                                float64 chain on every pixel                                                            */
/* all three merge entry points: */
#define HHSR_SENSOR_MONO 32  /* `mode: grey`: every sample goes to channel 0; the per-frame entry points and the generic
                                burst kernel leave channels 1, 2 of num / den as they are, the x2 tile kernel of
                                hhsr_merge_burst WRITES them (0, or 0 / 0 = NaN with HHSR_MERGE_DIVIDE — what the reference's
                                three-channel accumulators hold for a monochrome burst); covs is [H][W][2][2] read at the position itself, cfa is ignored (may be NULL);
                                hhsr_merge_burst: scale 2 (ts % 16 == 0, even sizes) runs the LDS-staged x2 tile kernel
                                with a per-pixel covariance window (HHSR_MERGE_LOCAL_MIN available), other scales the
                                generic kernel                                                                     */

/* ---- merge, Alg. 4 / Alg. 11 (merge.py; utils.py:62-120) --------------------------------------
 * hhsr_accumulate: one comp frame, num/den += (merge.py:291-434).
 * hhsr_accumulate_ref: the reference frame (merge.py:83-233); acc_rob = NULL disables the
 * accumulated-robustness widening (rad_max / max_multiplier / max_frame_count ignored).
 * `pitch` (>= W, odd allowed, raw 4-byte aligned) is the raw frame's alone: flow, covs, r, acc_rob, num and den are compact. */
int hhsr_accumulate(const float* raw, int H, int W, int pitch, const float* flow, int ny, int nx, int ts,
                    const float* covs, const float* r, const uint8_t cfa[4], double scale, int kflags,
                    float* num, float* den, int sH, int sW, void* stream);
int hhsr_accumulate_ref(const float* raw, int H, int W, int pitch, const float* covs,
                        const uint8_t cfa[4], double scale, int kflags,
                        const float* acc_rob, int rad_max, double max_multiplier, double max_frame_count,
                        float* num, float* den, int sH, int sW, void* stream);
int hhsr_divide(float* num, const float* den, int64_t n, void* stream);   /* num /= den */
int hhsr_add(float* A, const float* B, int64_t n, void* stream);          /* A += B */

/* Fused burst merge: for every HR pixel, sum the contributions of `n_frames` comp frames with the
 * accumulators held in registers (same left-to-right float32 order as n calls of hhsr_accumulate),
 * then optionally add the reference frame and normalise.  HOST arrays of device pointers.
 * Output rows [row0, row0 + nrows) are processed and num / den point at row0 (slabs for the multi-GPU
 * reduce-scatter; row0 = 0, nrows = sH for the whole image).
 * lr_row_offset: 0 for whole frames.  For a SUB-IMAGE (rows [offset, offset + H) of a larger frame: the row slabs of
 * the multi-GPU path) the raw row this image starts at — a multiple of ts and of 2 with an integer offset * scale:
 * sampling positions are then evaluated in full-frame coordinates, so their float64 / float32 roundings (merge.py:113-114
 * keeps idx / scale in float32) and therefore the results do not depend on how the frame was split.
 * acc_r (optional, float32 [H][W], integer scales only) receives sum_n r_n — the accumulated robustness of
 * super_resolution.py:158-159 — at no extra HBM traffic (+= with HHSR_MERGE_LOAD_ACC).
 * ONE `pitch` (>= W, odd allowed, 4-byte aligned bases) for all comp frames raws[] AND ref_raw; flows, covs, rs, ref_covs,
 * acc_r, num and den are compact.  For a sub-image, raws[n] / ref_raw point at the sub-image's first row inside the
 * full frame (pitch unchanged) and the other arrays at their matching rows.
 * Which kernel runs: hhsr_merge_plan_query below.
 * flags: */
#define HHSR_MERGE_LOAD_ACC 1   /* start from the existing num/den instead of zero          */
#define HHSR_MERGE_DO_REF 2     /* add the reference frame (ref_raw/ref_covs) after the comps */
#define HHSR_MERGE_DIVIDE 4     /* write num/den into num                                    */
#define HHSR_MERGE_STORE_DEN 8  /* also store den                                            */
#define HHSR_MERGE_LOCAL_MIN 16 /* rs[] hold the thresholded maps R of hhsr_rob_frame; their 5x5 clamp-border minimum
                                   (robustness.py:641-686, hhsr_local_min5) is taken inside the merge.  Only with the
                                   x2 kernels (scale 2, ts % 16 == 0, sH = 2 H, sW = 2 W, row0 % 32 == 0) and the
                                   x3 kernel (scale 3, Bayer cfa, W % 4 == 0, row0 % 48 == 0); float32 weights, no
                                   HHSR_MERGE_FORCE_GENERIC / _TILE; error -3 otherwise.                             */
int hhsr_merge_burst(const float* const* raws, const float* const* flows, const float* const* covs,
                     const float* const* rs, int n_frames, int H, int W, int pitch,
                     int ny, int nx, int ts, const float* ref_raw, const float* ref_covs,
                     const uint8_t cfa[4], double scale, int kflags, int flags,
                     float* num, float* den, float* acc_r, int sH, int sW, int row0, int nrows,
                     int lr_row_offset, void* stream);

/* Kernel choice of hhsr_merge_burst: what a launch with the same n_frames, H, W, ts, cfa (HOST), scale, kflags, flags, sH, sW,
 * row0 and nrows does, decided by the code the launch itself runs.  num_align / den_align: byte alignment of the launch's
 * num / den (16 or a multiple: 16-byte aligned; den_align counts only with HHSR_MERGE_STORE_DEN).  Host only: no HIP call,
 * usable without a device.  Invalid arguments return -1 as in the launch.  out (HOST, n >= HHSR_MERGE_PLAN_LEN values):
 *   [0] the kernel family.  With float32 weights, scale 2 and scale 3 with a BAYER cfa (red and blue on one diagonal, green on
 *       the other), ts % 16 == 0 and even / exact output sizes run the wave-per-parity-class kernels (three channel
 *       accumulators per sub-pixel; scale 3, which also needs W % 4 == 0 and 16-byte aligned outputs: frames whose window
 *       leaves the image are evaluated by the same code with border masks); other 2 x 2 colour layouts, unaligned outputs and
 *       monochrome sensors at scale 2 the first-generation x2 kernels; other integer scales with (ts scale) % 16 == 0 the
 *       16 x 16 tile kernel; everything else (non-integer scales, HHSR_WEIGHT_F64, no comp frame, a row0 off the
 *       family's grid, monochrome at other scales) the per-pixel kernel
 *   [1] position arithmetic of the float32 kernels at this scale: HHSR_MERGE_GEOM_P2 = idx / scale is exact in float32
 *       (scales 1, 2, 4, 8), HHSR_MERGE_GEOM_F64 = evaluated in float64 (with HHSR_WEIGHT_F64 always in float64)
 *   [2] 1 = these arguments admit HHSR_MERGE_LOCAL_MIN, [3] 1 = they admit a link of hhsr_merge_burst_chain
 *   [4] output rows per workgroup row of the family's grid (1, 16, 32 or 48): row0 has to be a multiple for the family to run
 *   [5] / [6] the grid's x / y size
 *   [7] what the launch returns for `flags` before it enqueues anything: 0, or -3 (HHSR_MERGE_LOCAL_MIN or a chain link asked
 *       for and not admitted; hhsr_last_error() then holds the launch's message). */
#define HHSR_MERGE_FAMILY_GENERIC 0  /* k_merge_burst: one thread per HR pixel                                 */
#define HHSR_MERGE_FAMILY_TILE 1     /* k_merge_burst_tile: 16 x 16 HR pixels through LDS                      */
#define HHSR_MERGE_FAMILY_X2V1 2     /* k_merge_burst_quad: first-generation x2                                */
#define HHSR_MERGE_FAMILY_X2_MONO 3  /* its monochrome form                                                    */
#define HHSR_MERGE_FAMILY_X2 4       /* k_merge_x2                                                             */
#define HHSR_MERGE_FAMILY_X3 5       /* k_merge_xs<3>                                                          */
#define HHSR_MERGE_GEOM_F64 0
#define HHSR_MERGE_GEOM_P2 1
#define HHSR_MERGE_PLAN_LEN 8
int hhsr_merge_plan_query(int n_frames, int H, int W, int ts, const uint8_t cfa[4], double scale, int kflags, int flags,
                          int sH, int sW, int row0, int nrows, int num_align, int den_align, int32_t* out, int n);

/* The fused x2 merge as a CHAIN of launches for bursts whose last frames arrive late (frames crossing PCIe: the early links
 * run while the late frames upload), bit-identical to ONE hhsr_merge_burst over all frames.  Every link gets the frames
 * that have arrived so far, raws[0 .. n_frames), of which the first n_done were merged by the links before it:
 *   first link   flags = HHSR_MERGE_STORE_CLASSES, n_done = 0: frames [0, n_frames) are merged into the kernel's
 *                parity-class accumulators, which are parked in class_acc (hhsr_merge_chain_bytes(H, W) bytes);
 *   middle link  flags = HHSR_MERGE_LOAD_CLASSES | HHSR_MERGE_STORE_CLASSES: restore, add frames [n_done, n_frames), park;
 *   last link    flags = HHSR_MERGE_LOAD_CLASSES | the flags of the single launch (DO_REF, DIVIDE, ...): restore, add the
 *                remaining frames, the reference frame, normalise, write the image (and acc_r).
 * (+ HHSR_MERGE_LOCAL_MIN in every link if the single launch had it.)  Tiles in which a window of ANY frame leaves the
 * image (they run a per-pixel code path: ~2 % at 12 MP) are skipped by the storing links and computed from the first
 * frame on by the last link, so every tile runs exactly the instruction sequence of the single launch.
 * Only with the wave-per-class x2 kernel (scale 2, ts % 16 == 0, sH = 2 H, sW = 2 W, float32 weights, Bayer, whole image);
 * error -3 otherwise. */
#define HHSR_MERGE_STORE_CLASSES 32
#define HHSR_MERGE_LOAD_CLASSES 64
size_t hhsr_merge_chain_bytes(int H, int W);
int hhsr_merge_burst_chain(const float* const* raws, const float* const* flows, const float* const* covs,
                           const float* const* rs, int n_frames, int H, int W, int pitch,
                           int ny, int nx, int ts, const float* ref_raw, const float* ref_covs,
                           const uint8_t cfa[4], double scale, int kflags, int flags,
                           float* num, float* den, float* acc_r, int sH, int sW,
                           float* class_acc, int n_done, void* stream);

/* ---- burst front end (utils_dng.py:149-160) ------------------------------------------------
 * Sensor counts uint16 [n_frames][H][pitch] -> normalised, white-balanced float32 [n_frames][H][W]:
 * v = (float32(count) - black[c]) / (white - black[c]); v *= wb[c] / wb[1], c = cfa[(y&1)*2 + (x&1)], in the
 * reference's float32 arithmetic (bit-identical to its NumPy expression, whatever the pitch: with W and pitch both
 * multiples of 8 a thread converts 8 counts with one 16-byte load, otherwise count by count — the same operations).
 * black_levels / white_balance: HOST double[3] indexed by colour (R, G, B); raw and out 16-byte aligned (error -1
 * otherwise); frame n starts at raw + n * H * pitch; out is compact. */
int hhsr_normalize_raw_u16(const uint16_t* raw, int n_frames, int H, int W, int pitch, const uint8_t cfa[4],
                           const double* black_levels, double white_level, const double* white_balance,
                           float* out, void* stream);

/* Packed sensor counts uint8 -> the same normalised float32 [n_frames][H][W], without widening them to uint16 on the
 * host first.  No counterpart in the reference (rawpy unpacks on the CPU).  p is a B-bit count, b the bytes of a group:
 *   HHSR_PACK_MIPI10  MIPI CSI-2 RAW10, groups of 4 pixels in 5 bytes:  b[i] = p[i] >> 2 (i < 4),
 *                     b[4] = (p[0] & 3) | (p[1] & 3) << 2 | (p[2] & 3) << 4 | (p[3] & 3) << 6;      row: 5 ceil(W / 4) bytes
 *   HHSR_PACK_MIPI12  RAW12, groups of 2 pixels in 3 bytes:  b[i] = p[i] >> 4 (i < 2),
 *                     b[2] = (p[0] & 15) | (p[1] & 15) << 4;                                       row: 3 ceil(W / 2) bytes
 *   HHSR_PACK_MIPI14  RAW14, groups of 4 pixels in 7 bytes:  b[i] = p[i] >> 6 (i < 4), then the 24-bit value
 *                     (p[0] & 63) | (p[1] & 63) << 6 | (p[2] & 63) << 12 | (p[3] & 63) << 18 in b[4], b[5], b[6],
 *                     least significant byte first;                                                row: 7 ceil(W / 4) bytes
 *   HHSR_PACK_BE10 / _BE12 / _BE14  uncompressed TIFF / DNG, BitsPerSample B, FillOrder 1: the row is ONE bit stream,
 *                     pixel x is its bits [x B, (x + 1) B) counted from the most significant bit of byte 0, most
 *                     significant bit of the count first; every row starts on a byte.               row: ceil(W B / 8) bytes
 *   e.g. the 10-bit counts 3FF 000 155 2AA 001 are  FF 00 55 AA 93 | 00 00 00 00 01  as MIPI10 (the second group's three
 *   padding pixels 0) and  FF C0 05 56 AA 00 40  as BE10.
 * Row y of frame n starts at raw + n * frame_bytes + y * row_bytes (frame_bytes is not read when n_frames == 1); out is
 * compact.  v = (float32(p) - black[c]) / (white - black[c]) * (wb[c] / wb[1]) with the constants cast as in
 * hhsr_normalize_raw_u16 and no contraction: bit-identical to that entry point on the unpacked counts.  The padding
 * pixels of a row's last group, the bits and bytes behind its last pixel and the bytes between rows and frames are not
 * interpreted (bytes behind the last group / the last bit's byte are not read); nothing outside out[0 .. n H W) is
 * written.  raw, row_bytes and frame_bytes need no alignment and the result does not depend on theirs: a thread
 * converts 16 pixels — B / 2 dwords — with dword loads where its row starts on a dword, byte by byte otherwise and for
 * the last W % 16 pixels of a row.  out is 16-byte aligned.  The fast path (measured: profiles/packed_raw.txt) needs
 * BOTH every row on a dword — raw, row_bytes and frame_bytes multiples of 4; the minimal row_bytes is not one at every
 * width, e.g. 5005 bytes for 4004 MIPI10 pixels: pad the rows — AND W % 4 == 0, with which the float4 stores of a
 * workgroup are contiguous.  Any other row is read byte by byte and any other W stored pixel by pixel, 64 bytes apart
 * from lane to lane: the same bits, several times the time.  Error -1: a null pointer, an unknown packing, n_frames, H
 * or W <= 0, n_frames or H > 65535, W > INT32_MAX - 4096, row_bytes below the table's value, frame_bytes < H row_bytes (n_frames > 1),
 * cfa[k] > 2, white_level == black_levels[c], white_balance[1] == 0, a misaligned out.
 * hhsr_packed_row_bytes is host-only (no HIP call): the table's row bytes; error -1 for W <= 0 or an unknown packing. */
#define HHSR_PACK_MIPI10 1
#define HHSR_PACK_MIPI12 2
#define HHSR_PACK_MIPI14 3
#define HHSR_PACK_BE10 4
#define HHSR_PACK_BE12 5
#define HHSR_PACK_BE14 6
int hhsr_normalize_raw_packed(const uint8_t* raw, int n_frames, int H, int W, int64_t row_bytes, int64_t frame_bytes,
                              int packing, const uint8_t cfa[4], const double* black_levels, double white_level,
                              const double* white_balance, float* out, void* stream);
int hhsr_packed_row_bytes(int W, int packing, int64_t* bytes_out);

/* ---- DNG linearization: LinearizationTable, BlackLevelDeltaH / V and GainMap opcodes ----------------------------------
 * hhsr_normalize_raw_u16 with the part of the DNG specification called "mapping raw values to linear reference values"
 * applied on the way (dng.parse_dng(linearization=True) reads the tags; no counterpart in the reference, whose rawpy
 * raw_image has none of it applied).  uint16 [n_frames][H][row_stride] -> float32 [n_frames][H][W], compact.  float32
 * arithmetic, every operation rounded once, no contraction; the map coordinates in float64 (IEEE division in both).
 * tests/dng_linearize_ref.py is the NumPy form, matched bit for bit.  For pixel (y, x): k = (y & 1) * 2 + (x & 1),
 * c = cfa[k], and
 *   1. lin = table ? table[min(count, table_len - 1)] : count, cast to float32.
 *   2. b = (float32(black[c]) + delta_h[x]) + delta_v[y], a missing delta being 0.0f (added all the same);
 *      den = float32(white) - b;  v = (lin - b) / den.
 *   3. where position k has a map m with PV x PH points:
 *        u = ((y + 0.5) / H - origin_v) / spacing_v  in float64; PV == 1 or u <= 0: r0 = r1 = 0, fv = 0;
 *        u >= PV - 1: r0 = r1 = PV - 1, fv = 0; otherwise r0 = floor(u), r1 = r0 + 1, fv = float32(u - r0);
 *        the same along x with W, origin_h, spacing_h, PH gives c0, c1, fh;
 *        t0 = m[r0][c0] * (1 - fv) + m[r1][c0] * fv;  t1 the same at c1;  g = t0 * (1 - fh) + t1 * fh;  v = v * g.
 *      A position without a map is not multiplied.
 *   4. v = v * float32(wb[c] / wb[1]).
 * No clipping, as in hhsr_normalize_raw_u16, whose bits this gives when table, deltas and maps are all absent and the
 * levels are integers (there den is float32(white - black[c]), rounded from the float64 difference; here it is the float32
 * difference of the rounded levels: equal whenever both levels are exact in float32).
 * The coordinate rule is the DNG specification's "relative coordinates" over the whole image with the pixel centre at
 * + 0.5, AS READ HERE: never compared with Adobe's DNG SDK, dng_validate, LibRaw or a camera's file.
 * table: DEVICE uint16[table_len], 1 .. 65536 entries, or NULL with table_len 0.  delta_h: DEVICE float32[W], delta_v:
 * DEVICE float32[H], either may be NULL.  maps: HOST, n_maps <= HHSR_MAX_GAIN_MAPS descriptors; gains: DEVICE
 * float32[gains_len] holding every map row-major at its `offset`.  Either ONE map with row_pitch = col_pitch = 1 and
 * top = left = 0, which covers every position, or maps with row_pitch = col_pitch = 2 and top, left in {0, 1}, at most one
 * per position top * 2 + left.  A map's spacing along an axis with one point is not read.
 * row_stride is the pitch of hhsr_normalize_raw_u16 (elements between rows of raw; frame n starts at
 * raw + n * H * row_stride): with W and row_stride multiples of 8 a thread converts 8 counts with one 16-byte load,
 * otherwise count by count, the same operations; tests/test_dng_linearize_gpu.py holds its padded and guarded cases.
 * Error -1: a null raw / cfa / black_levels / white_balance / out; n_frames, H or W <= 0; n_frames or H > 65535;
 * W > INT32_MAX - 2048; row_stride < W; raw or out not 16-byte aligned; white_balance[1] == 0; cfa[k] > 2; a table with
 * table_len outside 1 .. 65536 or table_len != 0 without one; n_maps outside 0 .. 4, or maps / gains NULL with n_maps > 0;
 * points outside 1 .. 64; an offset with which a map leaves gains[0 .. gains_len); a non-finite origin; a spacing that
 * is not finite and > 0 on an axis with more than one point; pitches other than 1, 1 / 2, 2; top or left outside what
 * the pitch allows; two maps for one position. */
#define HHSR_MAX_GAIN_MAPS 4
typedef struct hhsr_gain_map {
    int32_t top, left, row_pitch, col_pitch;
    int32_t points_v, points_h;
    double spacing_v, spacing_h, origin_v, origin_h;
    int64_t offset; /* of m[0][0] in gains, in floats */
} hhsr_gain_map;
int hhsr_linearize_raw_u16(const uint16_t* raw, int n_frames, int H, int W, int row_stride, const uint8_t cfa[4],
                           const double* black_levels, double white_level, const double* white_balance,
                           const uint16_t* table, int table_len, const float* delta_h, const float* delta_v,
                           const hhsr_gain_map* maps, int n_maps, const float* gains, int64_t gains_len, float* out,
                           void* stream);

/* ---- reference selection: the sharpness score of a burst's candidate base frames ---------------------------------------
 * The reference takes file 0 of the burst as its base frame (utils_dng.py:77); the burst pipelines the algorithm comes from
 * (HDR+; Wronski et al.) take the sharpest of the first few frames, scored by the gradients of the raw green channel.  No
 * counterpart in the reference.  The score, stated once (tests/sharpness_ref.py is its NumPy form):
 *
 *   frame     [H][W], H and W even; h = H / 2, w = W / 2.
 *   value     v(y, x): a float32 frame's value itself; for uint16 or packed counts float32(count), NOT normalised — only
 *             the order of a burst's frames matters, and black level, white level and green gain are common to them.
 *   green     Bayer: g(qy, qx) = (v_a + v_b) * 0.5f, a < b the two positions of the 2 x 2 CFA cell whose entry is 1, in cell
 *             order (row & 1) * 2 + (col & 1).  No CFA (cfa NULL, `mode: grey`): g = ((v00 + v01) + (v10 + v11)) * 0.25f.
 *   terms     dx = g(qy, qx + 1) - g(qy, qx) for qx < w - 1, dy = g(qy + 1, qx) - g(qy, qx) for qy < h - 1; a term is d * d,
 *             the float32 subtraction and the float32 multiplication, not contracted.
 *   score     the sum of all h (w - 1) + (h - 1) w terms in float64.  A 2 x 2 frame scores 0; NaN and Inf propagate.
 *
 * The order of the float64 additions is a function of (H, W) alone: a thread adds the terms of its 8 quads per quad row in
 * a fixed order, a wave its lanes and a workgroup its waves by a fixed tree, every workgroup stores one double into the
 * workspace and a second kernel adds a frame's partials in a fixed order.  No float64 atomics.  So a frame's score is
 * reproducible bit for bit and does not depend on its alignment, its row stride, n_frames, its place in `frames`, its
 * format (the same counts as float32, uint16 or packed bytes) or on which load path a row takes: 16-byte vectors (packed
 * rows: dwords) where the 16-pixel pieces of a wave's 1024 pixels are all whole and base and row_bytes are multiples of 16
 * (packed: of 4), a decision per piece and item-by-item reads elsewhere.  The order itself is not part of
 * the contract (it moves the score by float64 rounding: at most n_terms 2^-52 relative).
 *
 * hhsr_sharpness_workspace (host only, no HIP call): bytes of the partial sums, n_frames doubles per workgroup of 1008 x 64
 *   pixels; never smaller for a larger H, a larger W or more frames.
 * hhsr_frame_sharpness: frames HOST table of n_frames (1 .. HHSR_MAX_BATCH) DEVICE pointers, one shape and format; row y
 *   of frame n starts at (char*)frames[n] + y * row_bytes.  format: 0 float32, -1 uint16, or HHSR_PACK_* for packed uint8 rows
 *   (the layouts of hhsr_normalize_raw_packed, read by the same code).  cfa: HOST, 4 bytes, or NULL for a monochrome
 *   sensor.  scores: DEVICE double[n_frames].  workspace: DEVICE, 8-byte aligned, at least the bytes
 *   hhsr_sharpness_workspace reports; contents are scratch.  Every byte of a frame's rows is read once (a workgroup reads the
 *   16 pixels right of it and the 2 rows below each of its 4 bands once more, from cache: 1 / 63 and 1 / 8 of the frame);
 *   the bytes between a row's end and the next row are not read.
 *   Two launches on `stream`, no allocation, copy or synchronisation: capturable.
 *   Error -1, before any HIP call: a null pointer (cfa excepted), n_frames outside 1 .. HHSR_MAX_BATCH, H or W odd or <= 0,
 *   W > INT32_MAX - 2048 or H > 4194240 (the kernel's 32-bit pixel indices and its grid), a cfa without exactly two entries
 *   equal to 1 or with an entry above 2, an unknown format, row_bytes below the row's bytes (4 W, 2 W,
 *   hhsr_packed_row_bytes) or not a multiple of the item size, H row_bytes beyond int64, a frame pointer not aligned to its
 *   item (4, 2, 1 bytes), scores or workspace off 8 bytes, a workspace that is too small. */
int hhsr_sharpness_workspace(int H, int W, int n_frames, size_t* bytes);
int hhsr_frame_sharpness(const void* const* frames, int n_frames, int H, int W, int64_t row_bytes, int format,
                         const uint8_t* cfa, void* workspace, size_t workspace_bytes, double* scores, void* stream);

/* ---- noise profile: (alpha, beta) of a burst that brings none ---------------------------------------------------------------
 * The reference reads the two numbers of its noise model, variance = alpha x + beta on normalised raw values, from the DNG
 * NoiseProfile tag (super_resolution.py:232-238).  Arrays, .npz files, sensor counts and packed rows have no such tag: these
 * two entry points estimate the pair from the frames.  No counterpart in the reference.  The estimator, stated once
 * (tests/noise_profile_ref.py is its NumPy form):
 *
 *   frame     float32 [H][W], normalised and white-balanced (what main() receives), H and W even; h = H / 2, w = W / 2.
 *   value     u = v * inv_gain[p], one float32 multiplication, p = (row & 1) * 2 + (col & 1) the CFA position; inv_gain[p] is
 *             the float32 reciprocal of wb[cfa[p]] / wb[1] (all 1 for a monochrome sensor): the statistics are taken before
 *             the white balance, like the DNG tag, and a saturated pixel sits at u = 1 whatever its colour.
 *   tile      8 x 8 quads of ONE plane p (a 16 x 16 pixel block of the frame holds one tile of each plane), at multiples of 8
 *             quads; quads right of 8 (w / 8) or below 8 (h / 8) belong to no tile and are not read; no halo.
 *   counts    a tile counts if each of its 64 values satisfies 0 < u < 1 (NaN does not): no clipped or saturated tile.
 *   mean      m = s / 64, s the float64 sum of the 64 values: each row's 8 values are added left to right, then the 8 row
 *             sums top to bottom.
 *   residual  at the 36 interior quads, r = u(y, x) - 0.25f * ((u(y, x-1) + u(y, x+1)) + (u(y-1, x) + u(y+1, x))) in float32,
 *             not contracted.
 *   energy    e = float32(S / 45.0), S the float64 sum of the float32 products r * r in the same order (6 per row left to
 *             right, then the 6 row sums top to bottom); 45 = 36 x 1.25, the residual's variance gain for white noise.  A tile
 *             with e == 0 is dropped.
 *   bins      mean bin b = min(63, int(m * 64)); energy bin k = clamp((bits(e) >> 18) - ((127 - 32) << 5), 0, 1023), bits(e)
 *             the float's bit pattern: 32 octaves below 1 at 32 bins each; below 2^-32: bin 0, 1 and above: bin 1023.
 *   histogram uint32 [4 planes][64][1024] (1 MiB): one integer atomic add per tile, so the result does not depend on any order:
 *             the same bits for any row stride, alignment, split of the frames into calls (added up) and frame order.
 *
 * hhsr_noise_profile_hist: frames HOST table of n_frames (1 .. HHSR_MAX_BATCH) DEVICE pointers, one shape; row y of frame n
 *   starts at (char*)frames[n] + y * row_bytes.  cfa: HOST, 4 bytes, or NULL for a monochrome sensor (only checked here: the
 *   planes are positions).  inv_gain: HOST float[4].  hist: DEVICE, 1 MiB, zeroed on `stream` by the call, then the tiles of
 *   all frames of the call are added.  A frame smaller than one tile has none: the histogram stays zero, return 0.  Every byte
 *   of a whole 16 x 16 block is read once, with 16-byte loads where frames[n] and row_bytes are multiples of 16 and dword loads
 *   elsewhere; nothing else is read.  One memset node and one launch, no allocation, copy or synchronisation: capturable.
 *   Error -1, before any HIP call: a null pointer (cfa excepted), n_frames outside 1 .. HHSR_MAX_BATCH, H or W odd or <= 0,
 *   H > 16 * 65535 + 15 (the grid), W > INT32_MAX / 4, row_bytes < 4 W or not a multiple of 4, H row_bytes beyond int64, a
 *   frame pointer or hist off 4 bytes, a cfa entry above 2.
 * hhsr_noise_profile_fit (host only, no HIP call): hist HOST [4][64][1024].  Per colour c (R, G, B) the planes with
 *   cfa[p] == c are added (green: its two); cfa NULL: all four, one pair, written to all three.  Per mean bin with n_b >=
 *   min_tiles (>= 1; 16 is a good default) tiles: x_b = (b + 0.5) / 64, y_b = the median of the bin's energy histogram: at the
 *   first k whose cumulative count reaches 0.5 n_b, interpolated linearly between the bin's edges, the floats with the bits
 *   (k + ((127 - 32) << 5)) << 18 and that plus 1 << 18: y_b = lo + (0.5 n_b - count below k) / count[k] * (hi - lo).
 *   y = alpha x + beta by least squares in float64 with the weights n_b / y_b^2; a negative intercept is refitted with
 *   beta = 0, otherwise a negative slope with alpha = 0.  alpha_beta: HOST double[8] = (alpha, beta) of R, G, B and their mean
 *   (the reference's rule for the three pairs of the DNG tag, super_resolution.py:236-238); bins_used: HOST int[3], the usable
 *   bins per colour, written in every case.  Error -3: a colour with fewer than 2 usable bins (hhsr_last_error names the first).
 *   Known bias, not corrected: the median of a tile energy lies 1 - 2 % below the variance, and texture finer than a tile
 *   counts as noise: on a textured scene the result is an upper bound. */
int hhsr_noise_profile_hist(const void* const* frames, int n_frames, int H, int W, int64_t row_bytes, const uint8_t* cfa,
                            const float* inv_gain, uint32_t* hist, void* stream);
int hhsr_noise_profile_fit(const uint32_t* hist, const uint8_t* cfa, int min_tiles, double* alpha_beta, int* bins_used);

/* ---- white balance: gains of a burst that brings none ----------------------------------------------------------------------
 * The reference multiplies rawpy's camera_whitebalance (DNG AsShotNeutral) into every frame (utils_dng.py:149-160).  Counts
 * that come from a sensor interface have no such tag: these two entry points estimate the gains (R, 1, B) from the counts,
 * the black and white levels and the CFA pattern.  No counterpart in the reference.  The estimator, stated once
 * (tests/white_balance_ref.py is its NumPy form); every step is exact integer arithmetic or ONE correctly rounded float32
 * operation, not contracted:
 *
 *   frame     counts [H][W], uint16 or packed rows (the layouts of hhsr_normalize_raw_packed), H and W even, NOT normalised.
 *   tile      the whole 16 x 16 pixel blocks at (16 i, 16 j); rows and columns behind the last whole tile are not read.
 *   sums      per colour c, S_c = the integer sum of the tile's counts at the CFA positions of colour c; n_c = 64 for R and
 *             B, 128 for G (S_c <= 128 x 65535 < 2^24: float32(S_c) is exact).
 *   clipping  a tile is dropped if any of its counts is >= sat_c of its colour, sat_c = ceil(black_c + 15 / 16 (white -
 *             black_c)) in float64: a clipped channel fakes a chroma.
 *   means     m_c = (float32(S_c) / float32(n_c) - float32(black_c)) / float32(white - black_c), the casts of
 *             hhsr_normalize_raw_u16.  A tile is dropped unless every m_c >= 1 / 64 (which removes non-positive means).
 *   chroma    q_r = m_G / m_R, q_b = m_G / m_B: the gains that would make this tile grey.
 *   bins      u = (bits(q_r) >> 18) - ((127 - 2) << 5), v the same of q_b, bits(q) the float's bit pattern: 32 bins per
 *             octave from 1 / 4 on.  A tile is dropped unless 0 <= u, v < HHSR_WB_BINS: gains in [1 / 4, 16).
 *   histogram uint32 [192][192] (144 KiB), hist[u][v] += 1: integer adds, so the result does not depend on any order: the same
 *             bits for any row stride, alignment, format of the same counts, split of the frames into calls (added up) and
 *             frame order.
 *
 * hhsr_white_balance_hist: frames HOST table of n_frames (1 .. HHSR_MAX_BATCH) DEVICE pointers, one shape and format; row y
 *   of frame n starts at (char*)frames[n] + y * row_bytes.  format: -1 uint16 or HHSR_PACK_*, as for hhsr_frame_sharpness;
 *   0 (float32) is refused: normalised float frames are already white-balanced by this library's convention.  cfa: HOST,
 *   4 bytes, required (a monochrome sensor has no white balance), one entry 0, two 1, one 2.  black_levels: HOST double[3]
 *   by colour.  hist: DEVICE, zeroed on `stream` by the call, then the tiles of all frames of the call are added.  A frame
 *   smaller than one tile has none: the histogram stays zero, return 0.  Every byte of a whole tile is read once — uint16
 *   with 16-byte loads where frames[n] and row_bytes are multiples of 16 and count by count elsewhere, packed rows by the
 *   reader of hhsr_normalize_raw_packed (dwords where the row starts on one, bytes elsewhere) — and nothing else is read.
 *   One memset node and one launch, no allocation, copy or synchronisation: capturable.
 *   Error -1, before any HIP call: a null pointer, n_frames outside 1 .. HHSR_MAX_BATCH, the sizes hhsr_frame_sharpness
 *   refuses (H or W odd or <= 0, W > INT32_MAX - 2048), H > 16 * 65535 + 15 (the grid), format 0 or unknown, a cfa that is
 *   not one R, two G and one B, row_bytes below the row's bytes (2 W, hhsr_packed_row_bytes) or odd for uint16, H row_bytes
 *   beyond int64, a uint16 frame pointer off 2 bytes, hist off 4 bytes, white_level <= black_levels[c].
 * hhsr_white_balance_fit (host only, no HIP call): hist HOST [192][192].  In float64, bins visited in the order (u, v), on the
 *   bin centres c_k = log2(2^(k / 32 - 2, floored) (1 + ((k mod 32) + 0.5) / 32)):
 *   1. N = the sum of all counts; N < min_tiles (>= 1; 16 is a good default): error -3 (the frame is too small, black or
 *      clipped), white_balance = (1, 1, 1), tiles = (N, 0).
 *   2. (cu, cv) = the count-weighted centroid of all bins' centres: a geometric grey world.
 *   3. four times: (cu, cv) = the centroid of the bins whose centre (c_u, c_v) has (c_u - cu)^2 + (c_v - cv)^2 <= 0.25 —
 *      within half an octave, which throws out a large coloured object; a gate that holds no tile ends the loop and the
 *      estimate stays.
 *   4. white_balance: HOST double[3] = (2^cu, 1, 2^cv); tiles: HOST int64[2] = (N, the tiles inside the last gate; 0 if it was
 *      empty).
 *   Grey world's own assumption — the scene's balanced channel means are equal — is not checked and cannot be. */
#define HHSR_WB_BINS 192
int hhsr_white_balance_hist(const void* const* frames, int n_frames, int H, int W, int64_t row_bytes, int format,
                            const uint8_t cfa[4], const double* black_levels, double white_level, uint32_t* hist,
                            void* stream);
int hhsr_white_balance_fit(const uint32_t* hist, int min_tiles, double white_balance[3], int64_t tiles[2]);

/* ---- after the path: frame-count denoisers, postprocess, orientation — on the device -------------
 * hhsr_frame_count_denoise: utils_image.py:174-309.  image / out float32 [H][W][3] (the merged image), acc_r float32
 * [ah][aw] (accumulated robustness).  kind 0 = median (strength_max = radius_max <= 7: the reference's 16 x 16 sample
 * buffer overflows beyond that, error -2), kind 1 = gauss (strength_max = sigma_max; window |i|, |j| <= ceil(3 sigma) —
 * the reference's range() of a float does not type under Numba, so the build defines it).  half_index 1 = the
 * reference's index int(round((y - 0.5) / (2 scale))) into acc_r, 0 = the nearest raw pixel, 2 = int(round(y / scale)),
 * the reference's `mode: grey` branch (utils_image.py:203-204, 260-261). */
int hhsr_frame_count_denoise(const float* image, float* out, int H, int W, const float* acc_r, int ah, int aw,
                             double scale, int kind, double strength_max, double max_frame_count, int half_index,
                             void* stream);
/* hhsr_postprocess: raw2rgb.py:206-250 — optional colour matrix cam2rgb (HOST float[9], row major; NULL = off) + clip,
 * optional unsharp mask (skimage.filters.unsharp_mask = scipy.ndimage.gaussian_filter, mode "reflect": DEVICE double
 * taps[2 radius + 1], rows first, float64 accumulation, float32 intermediate in tmp [H][W][3]; result = c + (c - blur)
 * amount), optional devignetting (raw2rgb.py:198-204), clip, optional gamma 1/2.2, clip; the result is stored at its
 * EXIF-oriented position (utils_image.py:12-55; orientation 5..8: out is [W][H][3]).  Tone mapping (do_tonemapping) sits between the
 * devignetting and the first clip: hhsr_post_expose + hhsr_mertens below, then this call with every earlier stage off. */
int hhsr_postprocess(const float* image, float* tmp, float* out, int H, int W, const float* cam2rgb, int do_sharpen,
                     double amount, const double* taps, int radius, int do_devignette, int do_gamma, int orientation,
                     void* stream);
/* float32 [H][W] plane (accumulated robustness) to its EXIF-oriented position (utils_image.py:12-55). */
int hhsr_orient_plane(const float* in, float* out, int H, int W, int orientation, void* stream);

/* ---- tone mapping (raw2rgb.py:153-170): exposure fusion of the finished image, then the smoothstep curve -------------
 * The reference builds uint8 exposures of the image at times (1, 0.5, 2), fuses them with cv2.createMergeMertens() and
 * applies 3 r^2 - 2 r^3.  OpenCV is not part of this build: the contract is OpenCV 4.x MergeMertens with its default
 * weights (contrast 1, saturation 1, exposure 0) restated operation by operation — tests/mertens_ref.py is the NumPy
 * form the kernels are tested against — and has not been compared with a cv2 run (PARITY.md).  All images here are
 * COMPACT (no pitch).
 *
 * hhsr_post_expose: hhsr_postprocess's colour matrix + clip, unsharp mask and devignetting, bit for bit, then instead
 * of clip / gamma / orientation the exposures e_i = rint(clip(image times[i], 0, 1) 255), half to even, uint8
 * [n][H][W][3] (skimage img_as_ubyte).  The image is NOT clipped before it is scaled, and the arithmetic has the
 * precision the image has upstream: float32, or float64 when do_devignette (float64 gain x float32 image).  times:
 * HOST double[n], 1 <= n <= HHSR_MAX_EXPOSURES.  A NaN pixel gives 0.  tmp as for hhsr_postprocess.
 *
 * hhsr_mertens: exposures uint8 [n][H][W][3] -> out float32 [H][W][3].
 *   I = float(e) * float(1 / 255);                       weight maps in float32, this association, no FMA:
 *   grey = (I0 0.299f + I1 0.587f) + I2 0.114f;  contrast = |(((g[y-1,x] + g[y,x-1]) + g[y,x] (-4)) + g[y,x+1]) + g[y+1,x]|
 *   (reflect-101 border);  mean = ((I0 + I1) + I2) float(1 / 3);  saturation = sqrt((d0 d0 + d1 d1) + d2 d2), d = I - mean;
 *   w = contrast saturation + 1e-12f;  wn_i = w_i / ((w_0 + w_1) + w_2 ...)   (sqrt and division correctly rounded).
 *   levels L = floor(log2(min(H, W))) (OpenCV: int(logf(float(min)) / logf(2.f)), which at a power of two depends on
 *   the platform's logf); Gaussian pyramids of I_i and wn_i (pyrDown: [1 4 6 4 1] / 16 per
 *   axis at 2 i, size (n + 1) / 2, reflect-101); out_l = sum_i (G_l - pyrUp(G_{l+1})) W_l + pyrUp(out_{l+1}), out_L =
 *   sum_i G_L W_L (pyrUp: out[2i] = (s[i-1] + 6 s[i] + s[i+1]) / 8, out[2i+1] = (s[i] + s[i+1]) / 2 per axis, s[-1] = s[1],
 *   s[n] = s[n-1]); out = out_0, through 3 r^2 - 2 r^3 when `smoothstep`.  On pixels whose three channels are equal
 *   after quantisation the saturation is 0 or one rounding error, so the weights there are decided by float32 rounding
 *   alone: that is why the association above is part of the contract.
 * weights_out: optional float32 [n][H][W], the normalised weights wn.  workspace: DEVICE scratch of at least the
 * `bytes` hhsr_tonemap_workspace reports (4-byte aligned), overlapping none of the other arguments (error -1).
 * hhsr_tonemap_workspace is host-only (no HIP call): bytes and pyramid levels L for an image. */
int hhsr_tonemap_workspace(int H, int W, int n, size_t* bytes, int* levels);
int hhsr_post_expose(const float* image, float* tmp, int H, int W, const float* cam2rgb, int do_sharpen, double amount,
                     const double* taps, int radius, int do_devignette, const double* times, int n, uint8_t* exposures,
                     void* stream);
int hhsr_mertens(const uint8_t* exposures, int n, int H, int W, void* workspace, size_t workspace_bytes,
                 float* weights_out, float* out, int smoothstep, void* stream);

/* ---- noise curves of the robustness noise model (fast_monte_carlo.py; super_resolution.py:252) ------------------------
 * std_curve / diff_curve, float64[1001] for brightness i / 1000, i = 0 .. 1000 — the tables hhsr_rob_sigma,
 * hhsr_ref_planes and hhsr_rob_frame read — from the sensor's noise profile (alpha, beta): for every brightness draw
 * n_patches pairs of 3 x 3 patches b + sqrt(alpha b + beta) N(0, 1) clipped to [0, 1]; sigma = mean over the pairs of
 * the patches' mean standard deviation, d = mean |difference of the two patch means| (fast_monte_carlo.py:44-84).  The
 * reference draws from an unseeded generator; here the stream is part of the contract (tests/noise_mc_ref.py is its
 * NumPy form), so a value depends on (alpha, beta, n_patches, seed, i) alone:
 *
 * random words   Philox4x32-10.  key (k0, k1) = (seed & 0xffffffff, seed >> 32); counter (c0, c1, c2, c3) = (patch pair
 *                p in 0 .. n_patches - 1, brightness index i, call k in 0 .. 4, 0) — the brightness INDEX, not its place
 *                in `levels`.  Ten times: (c0, c1, c2, c3) <- (hi(0xCD9E8D57 c2) ^ c1 ^ k0, lo(0xCD9E8D57 c2),
 *                hi(0xD2511F53 c0) ^ c3 ^ k1, lo(0xD2511F53 c0)) with hi / lo the halves of the 64-bit product, then
 *                (k0, k1) <- (k0 + 0x9E3779B9, k1 + 0xBB67AE85) mod 2^32.  The call's words are x0 .. x3 = c0 .. c3.
 * normals        per call two Box-Muller pairs, (x0, x1) then (x2, x3): u = ((x >> 8) + 0.5) 2^-24 for both words,
 *                r = sqrt(-2 ln u_first), theta = 2 pi u_second, z = (r cos theta, r sin theta).  Call k gives normals
 *                4k .. 4k + 3; of the 20 normals of a pair, 0 .. 8 are patch 1 (row major), 9 .. 17 patch 2, 18 and 19
 *                are unused.
 * patch pair     float32, no fused multiply-add, sums left to right, typed as the torch estimator of
 *                fast_monte_carlo.regular_MC: b = float32(i / 1000) (the quotient in float64), s = sqrt(b float32(alpha) +
 *                float32(beta)), p_j = min(max(b + s z_j, 0), 1); per patch m = (p_0 + .. + p_8) / 9,
 *                sd = sqrt(((p_0 - m)^2 + .. + (p_8 - m)^2) / 9); per pair 0.5 (sd_1 + sd_2) and |m_1 - m_2|.  The
 *                normals are float32 too (u, ln, sqrt, 2 pi u, cos, sin; precise logf / sincosf, not the fast intrinsics).
 * accumulation   both per-pair values are widened to float64, summed over the pairs and divided by n_patches.  The
 *                order of the additions is fixed — a workgroup of 256 threads owns a chunk of HHSR_NOISE_MC_CHUNK
 *                consecutive pairs of one level (a thread every 256th of them, then wave shuffles, then the four waves
 *                through LDS in ascending order) and stores one partial per (level, chunk); a second kernel adds a
 *                level's partials in ascending chunk order.  No atomics: the same arguments give the same bits on every
 *                run, whatever else the GPU does, and a level's value does not depend on which other levels are in the
 *                launch or where it stands among them.  The order itself is not part of the contract (it moves the
 *                result by float64 rounding only).
 *
 * hhsr_noise_mc_levels (host only, no HIP call): the brightness indices run_fast_MC simulates, ascending, into levels
 *   (HOST int32[n]) and their number into *n_out: with (xmin, xmax) = get_non_linearity_bound(alpha, beta, tol = 3) —
 *   xmin = 4.5 (alpha + sqrt(9 alpha^2 + 4 beta)), xmax = (B - sqrt(B^2 - 4 (1 + 9 beta))) / 2, B = 2 + 9 alpha, in
 *   float64 — imin = ceil(1000 xmin) + 1 and imax = floor(1000 xmax) - 1: 0 .. imin and imax .. 1000, or all 1001 when
 *   imin > 1000 or imax <= imin (the reference's fallback; also taken when a bound is NaN or imax > 999 — beta above about
 *   alpha — where the reference raises).
 *   *n_out is set even when n is too small (error -1 then: n = 1001 always suffices; levels may be NULL with n = 0).
 * hhsr_noise_mc_workspace (host only): bytes of the partial sums, 2 n_levels ceil(n_patches / HHSR_NOISE_MC_CHUNK) doubles.
 * hhsr_noise_mc: levels DEVICE int32[n_levels] in any order (an index outside 0 .. 1000 is clamped into it by the
 *   kernel: the host cannot see it) -> sigma, diff DEVICE double[n_levels] in the order of levels.  Asynchronous on
 *   `stream`: two launches, no allocation, copy or synchronisation, so it can be captured into a graph.  workspace:
 *   DEVICE, 8-byte aligned, at least the bytes hhsr_noise_mc_workspace reports; its contents are scratch.
 *   Error -1 (before any HIP call): a null pointer, n_levels outside 1 .. 1001, n_patches < 1, alpha or beta negative or
 *   not finite, a misaligned pointer, a workspace that is too small.
 * hhsr_noise_curves_fill (host only; every pointer HOST): std_curve[levels[k]] = sigma[k], diff_curve likewise; the
 *   indices between the two simulated runs 0 .. imin and imax .. 1000 are interpolated as interp_MC /
 *   run_fast_MC do (fast_monte_carlo.py:126-157, 200-212): for i = imin .. imax, BOTH ends included (their simulated values are
 *   replaced), nb = (i / 1000 - (imin - 1) / 1000) / ((imax + 1) / 1000 - (imin - 1) / 1000) and
 *   std_curve[i] = sqrt(nb (sigma_imax^2 - sigma_imin^2) + sigma_imin^2), diff_curve the same with d.  With all 1001 levels
 *   given it is a copy.  Error -1: a level outside 0 .. 1000 or given twice, levels that are not 0 .. imin and imax .. 1000. */
#define HHSR_NOISE_MC_CHUNK 2048  /* patch pairs per workgroup of hhsr_noise_mc */
int hhsr_noise_mc_levels(double alpha, double beta, int32_t* levels, int n, int32_t* n_out);
int hhsr_noise_mc_workspace(int n_levels, int n_patches, size_t* bytes);
int hhsr_noise_mc(const int32_t* levels, int n_levels, double alpha, double beta, int n_patches, uint64_t seed,
                  double* sigma, double* diff, void* workspace, size_t workspace_bytes, void* stream);
int hhsr_noise_curves_fill(const int32_t* levels, int n_levels, const double* sigma, const double* diff,
                           double* std_curve, double* diff_curve);

/* ---- integer output (run_handheld.py:132-159; utils_dng.py:208-215): the finished image as the samples a file holds ------
 * The reference copies the float32 image to the host and quantises it there: nan_to_num, clip(0, 1), then skimage
 * img_as_ubyte for a PNG or round(x 65535) for the 16-bit TIFF of its DNG export.  Here the device image is encoded
 * and only the integer samples cross the host link (3 or 6 instead of 12 bytes per RGB pixel).  One rule for both widths,
 * in float32 without contraction — the rule hhsr_post_expose applies to its exposures:
 *
 *   v = x, NaN -> 0 (+-inf behave as +-FLT_MAX);  v = min(max(v, 0), 1);  p = v * M, M = 255 or 65535, ONE float32
 *   multiply rounded once;  q = rint(p), half to even;  sample = q as uint8 / uint16 (0 <= q <= M always).
 *
 * tests/output_ref.py is its NumPy form.  It equals img_as_ubyte and utils_dng.py:212-215 on float32 input.
 *
 * hhsr_encode_image: image DEVICE float32, compact [H][W][channels], channels 1 or 3, 4-byte aligned.  out_channels ==
 *   channels, or 1: channel 0 alone (the `mode: grey` result, whose channels 1 and 2 are NaN).  bits 8 or 16.  Row y of the
 *   result starts at (char*)out + y * out_row_bytes and holds W * out_channels samples; the bytes between the end of a row
 *   and the start of the next are never written, nor is anything else outside the rows.  out is aligned to its sample
 *   size only (any byte for uint8); out_row_bytes is any value that holds a row.  The result does not depend on
 *   alignment or stride; the time does: every lane loads float4 and stores 16 bytes wherever the output is 16-byte
 *   aligned — a compact output (out_row_bytes == W * out_channels * bits / 8) is ONE run over the whole image, a padded
 *   one a run per row; the fewer than 16 bytes before and behind the aligned part of a run are stored sample by sample.
 *   With out_channels != channels, or an image that is not 16-byte aligned where the aligned part of a run begins, the
 *   loads are dwords; with 16 bits and an odd out_row_bytes every other row starts on an odd byte and is stored byte by
 *   byte.  Sample and byte indices are 64-bit; the launch has one workgroup per 4096 output bytes of a run.
 *   Error -1, before any HIP call: a null image or out, H or W <= 0, bits not 8 or 16, channels not 1 or 3, out_channels
 *   neither channels nor 1, out_row_bytes < W * out_channels * bits / 8 (or so large that the last row's end
 *   overflows), an image off 4 bytes or a 16-bit out off 2, out overlapping image, more than INT32_MAX workgroups (a
 *   compact uint8 image beyond 8.7e12 samples).
 * hhsr_encode_mask: the robustness mask of run_handheld.py:153-159 — acc_r DEVICE float32 [ah][aw], the accumulated
 *   robustness already oriented, -> out uint8 [mH][mW], rows out_row_bytes apart (>= mW; no alignment):
 *   out[y][x] = rule8(acc_r[min((y ah) / mH, ah - 1)][min((x aw) / mW, aw - 1)] / float32(n_comp)), integer division of
 *   64-bit products, the float32 division before the rule.  Upstream replicates three channels and resizes with OpenCV's
 *   INTER_NEAREST; OpenCV is not part of this build: the index rule above is the contract, it is OpenCV's for integer
 *   ratios, and it has not been compared with a cv2 run (PARITY.md).  Error -1: a null pointer, a size <= 0, n_comp < 1,
 *   out_row_bytes < mW, a misaligned acc_r, out overlapping acc_r, mH > 262140. */
int hhsr_encode_image(const float* image, int H, int W, int channels, int out_channels, void* out, int bits,
                      size_t out_row_bytes, void* stream);
int hhsr_encode_mask(const float* acc_r, int ah, int aw, int n_comp, uint8_t* out, int mH, int mW, size_t out_row_bytes,
                     void* stream);

/* ---- JPEG output (run_handheld.py: imsave = cv2.imwrite writes a JPEG for a `.jpg` path, on the host) --------------------
 * The finished image as a baseline sequential JPEG (ITU-T T.81, JFIF 1.02 container, 8 bits), encoded on the device: the
 * entropy-coded scan is left in device memory with its length in a device word, and 5 - 15 times fewer bytes than the
 * uint8 samples cross the host link.  The file is  header || scan[0 .. length) || FF D9.  tests/jpeg_ref.py is the NumPy /
 * Python form of everything below.
 *
 *   samples   the 8-bit rule of "integer output": NaN -> 0, clip to [0, 1], ONE float32 multiply by 255, rint half to even.
 *             The JPEG of an image is the JPEG of its uint8 encoding.  channels 1 or 3; out_channels == channels, or 1:
 *             channel 0 alone as a one-component (grey) file, the `mode: grey` result.
 *   colour    three components: JFIF full-range YCbCr with the T.871 coefficients, level shift included,
 *               Y = 0.299 R + 0.587 G + 0.114 B - 128,  Cb = -0.168736 R - 0.331264 G + 0.5 B,
 *               Cr = 0.5 R - 0.418688 G - 0.081312 B   (float32; nothing is rounded before the transform);
 *             one component: q - 128.
 *   sampling  4:4:4 only: an MCU is one 8 x 8 block of each component, in the order Y, Cb, Cr.
 *   edges     H or W that is no multiple of 8: the last column and the last row of samples are replicated into the padding.
 *   DCT       the 8 x 8 DCT-II of T.81 A.3.3 in float32 (here: separable, each 8-point pass split into its even and odd
 *             half); coefficient = rint(c / Q[k]) clamped to the baseline range, DC to [-1024, 1023], AC to [-1023, 1023].
 *   Q         T.81 K.1 (luma) and K.2 (chroma) scaled by the IJG rule for quality 1 .. 100: s = 5000 / quality (integer
 *             division) below 50, else 200 - 2 quality; Q = clamp((base s + 50) / 100, 1, 255) (integer division).
 *   Huffman   T.81 K.3 - K.6 as they stand; no optimisation pass.
 *   scan      ONE scan, MCUs interleaved, in raster order.  restart_mcus = Ri, 1 .. 65535: a DRI segment in the header and
 *             RSTm (m = 0, 1, .. 7, 0, ..) after every Ri MCUs except after the last; the DC prediction is 0 at the start of
 *             each interval; an interval's last byte is padded with 1-bits; every 0xFF byte of entropy-coded data, padding
 *             bytes included, is followed by 0x00.  Ri >= the number of MCUs: no DRI, no marker.
 *   limits    H, W <= 65535.
 *
 * Coefficients: int16 [n_mcu][out_channels][64], n_mcu = ceil(H / 8) ceil(W / 8) MCUs in raster order, a block's 64 values
 * in zig-zag order, the DC values raw (not differenced).
 *
 * hhsr_jpeg_header (host only, no HIP call): SOI, APP0 (JFIF 1.02, no units, 1 : 1, no thumbnail), one DQT segment per table,
 *   SOF0 (components 1, 2, 3, each 1 x 1), one DHT segment per table (DC luma, AC luma, then DC chroma, AC chroma with three
 *   components), DRI when restart_mcus < n_mcu, SOS — into out (HOST, out_capacity bytes); *length = the header's bytes (328 /
 *   334 for one component, 623 / 629 for three, without / with DRI), set also when out_capacity is too small (error -1 then).
 * hhsr_jpeg_workspace (host only): *coef_bytes = 128 n_mcu out_channels; *scratch_bytes = the bytes hhsr_jpeg_entropy needs
 *   (20 per restart interval, rounded up: offsets, sizes and the partial sums of their scan);
 *   *max_scan_bytes = 432 n_mcu out_channels + 2 (n_intervals - 1): no symbol is longer than a 16-bit code plus 11 magnitude
 *   bits (the longest code of K.3 - K.6 is 16 bits; a DC difference has at most 11 extra bits, an AC value 10), one symbol
 *   per coefficient at most (ZRL and EOB stand for coefficients that get none), so a block is at most 64 x 27 bits = 216
 *   bytes, an interval's padding completes a byte that is already counted, every byte may be 0xFF and then is doubled, and
 *   every interval but the last is followed by a 2-byte marker.
 * hhsr_jpeg_dct: image DEVICE float32, compact [H][W][channels], 4-byte aligned -> coef DEVICE int16, 16-byte aligned,
 *   coef_bytes >= what hhsr_jpeg_workspace reports.  One launch.
 * hhsr_jpeg_entropy: coef as above -> scan[0 .. capacity) DEVICE bytes (no alignment) and *length (DEVICE uint64, 8-byte
 *   aligned): the scan's length, ALWAYS written, whatever capacity is.  No byte outside [scan, scan + capacity) is ever
 *   written, whatever coef holds: every coefficient is clamped to the baseline range as it is read, so that no table index
 *   leaves its table and no block exceeds the bound above, and every store compares its position with capacity.  If *length >
 *   capacity the content of scan is unspecified (the caller retries with *length bytes; max_scan_bytes always suffices).
 *   scratch: DEVICE, 8-byte aligned, scratch_bytes >= what hhsr_jpeg_workspace reports; contents are scratch.  Five launches
 *   (size pass, three for the exclusive scan of the intervals' sizes, write pass); no atomics on device memory: the bytes
 *   are a function of the coefficients alone, the same on every run and every stream.
 * All four: error -1 before any HIP call for a null pointer, H or W <= 0 or > 65535, quality outside 1 .. 100, channels not
 *   1 or 3, out_channels neither channels nor 1 (where there is no image: not 1 or 3), restart_mcus outside 1 .. 65535, a
 *   misaligned buffer, buffers that overlap, a buffer smaller than stated.  No allocation, no synchronisation, no copy: every
 *   launch goes on `stream`, so the calls can be captured into a graph. */
int hhsr_jpeg_header(int H, int W, int out_channels, int quality, int restart_mcus, uint8_t* out, size_t out_capacity,
                     size_t* length);
int hhsr_jpeg_workspace(int H, int W, int out_channels, int restart_mcus, size_t* coef_bytes, size_t* scratch_bytes,
                        size_t* max_scan_bytes);
int hhsr_jpeg_dct(const float* image, int H, int W, int channels, int out_channels, int quality, int16_t* coef,
                  size_t coef_bytes, void* stream);
int hhsr_jpeg_entropy(const int16_t* coef, int H, int W, int out_channels, int restart_mcus, void* scratch,
                      size_t scratch_bytes, uint8_t* scan, size_t capacity, uint64_t* length, void* stream);

/* JPEG output, extended: 4:2:0 chroma subsampling and Huffman tables made for the image.  The four entry points above keep
 * their signatures and results; with subsampling 0 and spec NULL an _ex function gives exactly what its namesake gives.
 * tests/jpeg_ex_ref.py is the NumPy / Python form of everything below.
 *
 *   subsampling  0: 4:4:4, as above.  1: 4:2:0, out_channels == 3 only:
 *     MCU        16 x 16 pixels; mcux = ceil(W / 16), mcuy = ceil(H / 16); the last column and the last row are replicated
 *                up to the next multiple of 16.
 *     Y          exactly the Y of 4:4:4: the same float32 operations on the same samples, block for block.
 *     Cb, Cr     per pixel in float32 as above, unrounded; a chroma sample is 0.25f * ((c00 + c01) + (c10 + c11)) of its
 *                2 x 2 pixels (c00 c01 the upper row): libjpeg's h2v2 box filter without its integer rounding.  Nothing
 *                is rounded before the transform.
 *     blocks     coefficients int16 [n_mcu][6][64] in zig-zag order, in the order of T.81 A.2.3: Y(0,0), Y(0,1), Y(1,0),
 *                Y(1,1), Cb, Cr (Y(r,c): block row r, block column c of the MCU).  coef_bytes = 768 n_mcu.
 *     header     SOF0 sampling factors 0x22 for Y, 0x11 for Cb and Cr; the same quantisation tables.
 *     scan       the restart interval counts 16 x 16 MCUs.  The DC prediction runs per component through the interval in
 *                coding order: the first Y block of an MCU predicts from the fourth Y block of the MCU before it.
 *     limits     max_scan_bytes = 432 * 6 n_mcu + 2 (n_intervals - 1).
 *   spec         a Huffman table specification, HOST uint8_t [n_tables][16 + 256]: BITS (the number of codes of length 1 ..
 *                16), then HUFFVAL (the symbols, by code), zero-filled.  Row order DC luma, AC luma, DC chroma, AC chroma;
 *                n_tables = 2 with one component, otherwise 4.  NULL: K.3 - K.6.  A DC symbol is the category of the
 *                difference (0 .. 11), an AC symbol run << 4 | size, 0xF0 = ZRL, 0x00 = EOB.  A row is refused unless it
 *                holds 1 .. 256 symbols, none twice, DC symbols <= 11, and BITS is a prefix code by annex C in which no
 *                code is all 1-bits.
 *
 * hhsr_jpeg_header_ex (host only): hhsr_jpeg_header with the sampling factors of `subsampling` and the DHT segments of `spec`.
 * hhsr_jpeg_workspace_ex (host only): the sizes for `subsampling`; *scratch_bytes covers both hhsr_jpeg_entropy_ex (20 bytes
 *   per interval, rounded up) and hhsr_jpeg_histogram (8192 bytes per workgroup: one for every 256 blocks, at most 512).
 * hhsr_jpeg_dct_ex: hhsr_jpeg_dct for `subsampling`.  One launch.
 * hhsr_jpeg_histogram: coef -> counts, DEVICE uint64 [4][256], 8-byte aligned: counts[t][s] = how often the scan of these
 *   coefficients at this restart interval emits symbol s of table t (row order as in spec).  The counts depend on
 *   restart_mcus because the DC prediction restarts with the interval.  The call overwrites counts; with one component rows
 *   2 and 3 are zero.  Exact integers, the same whatever the order of the launch's workgroups.  scratch: DEVICE, 8-byte
 *   aligned.  Two launches (counts per workgroup in LDS, then the sum of the workgroups' tables); no atomics on device memory.
 * hhsr_jpeg_huffman (host only, HOST pointers): counts [n_tables][256] -> spec [n_tables][16 + 256] by T.81 K.2 with
 *   libjpeg's choices: a reserved symbol 256 of count 1, so that no code is all 1-bits; the two least non-zero counts are
 *   merged, ties going to the larger symbol index (the first of the two is searched over all symbols, the second over all
 *   others); lengths above 16 are shortened by Figure K.3; the reserved symbol is removed from the longest length in use;
 *   HUFFVAL is ordered by the length K.2 found (before the shortening), then by symbol.  Error -1 also for a table whose
 *   counts are all zero or sum to 2^64 or more; spec is written only when every table was built.
 * hhsr_jpeg_entropy_ex: hhsr_jpeg_entropy for `subsampling` with the tables of `spec`.  The host turns spec into code words
 *   (annex C) that travel as a by-value kernel argument of 544 words: no copy, no allocation, the call stays capturable, and
 *   spec may be freed on return.  If a block needs a symbol the tables do not have — tables built at another restart
 *   interval, for instance — *length = UINT64_MAX and the content of scan is unspecified; still no byte outside
 *   [scan, scan + capacity) is written.  Five launches, as hhsr_jpeg_entropy.
 * All: error -1 before any HIP call for what the four entry points above refuse, subsampling outside 0 .. 1, subsampling 1
 *   with out_channels != 3, n_tables not 2 or 4, an invalid row of spec. */
int hhsr_jpeg_header_ex(int H, int W, int out_channels, int quality, int restart_mcus, int subsampling, const uint8_t* spec,
                        uint8_t* out, size_t out_capacity, size_t* length);
int hhsr_jpeg_workspace_ex(int H, int W, int out_channels, int restart_mcus, int subsampling, size_t* coef_bytes,
                           size_t* scratch_bytes, size_t* max_scan_bytes);
int hhsr_jpeg_dct_ex(const float* image, int H, int W, int channels, int out_channels, int quality, int subsampling,
                     int16_t* coef, size_t coef_bytes, void* stream);
int hhsr_jpeg_histogram(const int16_t* coef, int H, int W, int out_channels, int subsampling, int restart_mcus,
                        uint64_t* counts, void* scratch, size_t scratch_bytes, void* stream);
int hhsr_jpeg_huffman(const uint64_t* counts, int n_tables, uint8_t* spec);
int hhsr_jpeg_entropy_ex(const int16_t* coef, int H, int W, int out_channels, int restart_mcus, int subsampling,
                         const uint8_t* spec, void* scratch, size_t scratch_bytes, uint8_t* scan, size_t capacity,
                         uint64_t* length, void* stream);

/* ---- PNG output (run_handheld.py: imsave writes a PNG for a `.png` path, on the host) ------------------------------------
 * The finished image as a PNG file (ISO/IEC 15948, one IDAT chunk, no interlace), filtered and deflate-coded on the device:
 * the file's bytes are a function of the image and the options, and only counts, three result words and the file cross the
 * host link.  The file is  head || deflate[0 .. length) || tail.  tests/png_ref.py is the NumPy / Python form of all of it.
 *
 *   samples      exactly hhsr_encode_image's: rint(clip(nan_to_num(x), 0, 1) * M), half to even, M = 255 (bits 8) or 65535
 *                (bits 16, stored big-endian).  channels 1 or 3; out_channels == channels, or 1: channel 0 alone.  Colour
 *                type 2 (out_channels 3) or 0; bpp = out_channels * bits / 8.
 *   filtered     N = H (1 + W bpp) bytes: per row its filter type, then its bytes filtered by PNG 9.2: None (0), Sub (1),
 *                Up (2), Average (3), Paeth (4), on bytes, modulo 256; the bytes left of a row and above row 0 are 0.
 *                `filter` 0 .. 4: that type on every row.  5: adaptive, libpng's heuristic — per row, for each of the five
 *                types the sum over the row's filtered bytes v of (v < 128 ? v : 256 - v); the least sum wins, ties go to
 *                the lowest type.  Rows are independent: the row above is quantised from the image again.
 *   counts       uint64 [256]: how often each byte value occurs in `filtered` (filter types included).  The caller adds
 *                counts[256] = the number of intervals (one end-of-block symbol each) before hhsr_png_huffman.
 *   spec         HOST uint8_t [HHSR_PNG_SPEC_BYTES]: [0, 257) the code lengths of the literal / end symbols 0 .. 256
 *                (0: no code); [257] 0; [258, 260) the bit count of the block header, little-endian; [260, ...) the
 *                header's bits, LSB first, zero-filled: BFINAL 0, BTYPE 10, HLIT 257 codes, HDIST 2 codes of length 1
 *                (what zlib writes for a block without matches), HCLEN, the code-length code and the 259 lengths under it
 *                (RFC 1951 3.2.7).  Code words are canonical (RFC 1951 3.2.2).
 *   intervals    interval k covers filtered[k I, min((k + 1) I, N)), I = interval_bytes in 1 .. 2^20, and is one
 *                dynamic-Huffman block: the header, one code per byte, the end code; bits LSB first, Huffman codes MSB
 *                first (RFC 1951 3.1.1).  Every interval but the last has BFINAL 0 and is followed by an empty stored
 *                block — 000, zero bits to the byte boundary, 00 00 FF FF — so every interval starts on a byte; the last has
 *                BFINAL 1 and is zero-padded to the byte.
 *   result       DEVICE uint64 [3]: the length of the deflate stream; its CRC-32; the Adler-32 of `filtered`.  Both
 *                checksums are made on the device (per-interval remainders and sums, combined by a last launch).
 *   file         head: the signature, IHDR, the IDAT length (length + 6) and type, 78 01.  tail: the Adler-32, the CRC of
 *                the IDAT chunk — crc("IDAT" 78 01) combined with result[1] and the crc of the Adler-32's four bytes —
 *                and IEND.
 *   limits       the filtered stream and the bound below fit 2^31 - 1 bytes (one IDAT chunk), else error -1.
 *                max_deflate_bytes: a code of 8 bits for 255 of the 257 symbols and 9 bits for the two rarest is a prefix
 *                code, so the optimal code costs at most 8 T + 2 T / 257 bits for the T = N + n_int coded symbols (the two
 *                rarest of 257 symbols occur at most 2 T / 257 times together); an interval adds at most 3700 header bits
 *                (17 + 19 x 3 + 259 lengths of at most 7 + 7 bits), 3 bits, less than a byte of padding twice and 4 bytes:
 *                max_deflate_bytes = ceil((8 T + floor(2 T / 257) + 1) / 8) + 468 n_int.
 *
 * hhsr_png_workspace (host only): *stream_bytes = N; *scratch_bytes = what hhsr_png_filter (1024 bytes per workgroup, at most
 *   1024 of them) and hhsr_png_deflate (24 bytes per interval + 8 per 2048 intervals) need, the larger; *max_deflate_bytes.
 * hhsr_png_filter: image DEVICE float32, compact [H][W][channels], 4-byte aligned (16-byte aligned: 16-byte loads) ->
 *   filtered DEVICE, 16-byte aligned, filtered_bytes >= N, and counts DEVICE uint64 [256], 8-byte aligned, overwritten.
 *   scratch DEVICE, 8-byte aligned.  Exact integer counts, the same whatever the order of the workgroups; no atomics on
 *   device memory.  Two launches.
 * hhsr_png_huffman (host only, HOST pointers): counts [257] -> spec.  The lengths are optimal under the 15-bit limit
 *   (package-merge): zero counts get no code, every other symbol one, the code is complete.  Error -1 unless counts[256] and at
 *   least one byte value are counted and the counts sum to less than 2^59.
 * hhsr_png_deflate: filtered DEVICE (4-byte aligned, filtered_bytes = N in 1 .. 2^31 - 1) -> out[0 .. capacity) DEVICE bytes
 *   (no alignment) and result (8-byte aligned).  The code words and the header travel as a by-value kernel argument: no
 *   copy, no allocation, the call stays capturable, spec may be freed on return.  A stream longer than capacity is cut
 *   there — no byte outside [out, out + capacity) is written — and all three result words are still those of the whole stream.
 *   A byte value that spec gives no code: result[0] = UINT64_MAX, the rest unspecified.  The bytes and the result words are
 *   the same in every run and on every stream.  Six launches: sizes, the offsets scan (three), the write pass, the checksums.
 * hhsr_png_file_head / hhsr_png_file_tail (host only): the 43 and 20 bytes around the deflate stream; *length is set even when
 *   capacity is too small (error -1 then).  hhsr_png_crc_combine (host only): *crc = crc32(A || B) from crc32(A), crc32(B)
 *   and the length of B (any uint64).
 * All: error -1 before any HIP call for a null or misaligned pointer, dimensions <= 0, channels / out_channels / bits /
 *   filter / interval_bytes outside the above, a buffer smaller than stated, overlapping buffers, an invalid spec (a length
 *   above 15, a code that is not complete or lacks the end symbol, an impossible header length, BFINAL set). */
#define HHSR_PNG_SPEC_BYTES 768
int hhsr_png_workspace(int H, int W, int out_channels, int bits, int interval_bytes, size_t* stream_bytes,
                       size_t* scratch_bytes, size_t* max_deflate_bytes);
int hhsr_png_filter(const float* image, int H, int W, int channels, int out_channels, int bits, int filter,
                    uint8_t* filtered, size_t filtered_bytes, uint64_t* counts, void* scratch, size_t scratch_bytes,
                    void* stream);
int hhsr_png_huffman(const uint64_t* counts, uint8_t* spec);
int hhsr_png_deflate(const uint8_t* filtered, size_t filtered_bytes, int interval_bytes, const uint8_t* spec,
                     void* scratch, size_t scratch_bytes, uint8_t* out, size_t capacity, uint64_t* result, void* stream);
int hhsr_png_file_head(int H, int W, int out_channels, int bits, uint64_t deflate_len, uint8_t* buf, size_t capacity,
                       size_t* length);
int hhsr_png_file_tail(uint32_t deflate_crc, uint64_t deflate_len, uint32_t adler, uint8_t* buf, size_t capacity,
                       size_t* length);
int hhsr_png_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t* crc);

/* ---- DNG input: lossless JPEG (DNG Compression 7; ITU-T T.81 Annex H, SOF3) ----------------------------------------------
 * No counterpart in the reference, whose frames rawpy / LibRaw decode on one CPU core before anything is uploaded.  Each
 * tile or strip of a DNG is one independent stream: SOI, marker segments, one scan, EOI.  Python's dng.py parses the
 * container and drives the five entry points below; csrc/hhsr_ljpeg_core.h is the one implementation of the stream rules,
 * compiled for the host and for the kernel.
 *
 * hhsr_ljpeg_parse (host only, no HIP call): the stream's bytes -> *info.  Marker segments are walked by their lengths,
 *   each inside the stream.  SOF3: P (2..16), Y, X (>= 1), Nf (1..4), per component H = V = 1 and distinct ids.  DHT: class 0,
 *   id 0..3, 1..17 values each <= 16, code lengths with Kraft sum <= 1; bits[id] / values[id] / n_values[id] hold them.
 *   SOS: all Nf components in frame order, table[c] the DHT id of component c (it must be present), predictor 1..7.
 *   data_offset / data_length: the entropy-coded bytes, from behind SOS to the first marker (FF followed by a byte
 *   other than 00) or the stream's end.  Refused, error -1, hhsr_last_error() naming it: a restart interval (DRI != 0) or
 *   restart marker, a point transform != 0, a second scan (or a scan that holds fewer than Nf components), any SOF other
 *   than SOF3, DAC, and every violation of the above.  APPn, COM and other segments are skipped by their length.
 * hhsr_ljpeg_tables (host only): n (bits[16], values[17]) pairs, bits at bits + 16 i and values at values + 17 i -> the
 *   decode tables out[i] (HOST): lookup[b] for the next HHSR_LJPEG_LOOKUP_BITS bits b of the stream is len << 8 | SSSS of
 *   the code of len <= 8 bits that b starts with, 0 when there is none; then the ladder of T.81 F.2.2.3 for len 9..16:
 *   the first len with (next len bits) <= maxcode[len] decodes to values[(next len bits) + valoff[len]].  maxcode[len] is
 *   -1 where no code has that length.  Error -1 for lengths that are no prefix code, no value, more than 17, a value > 16.
 * hhsr_ljpeg_workspace (host only): sets segs[i].line_offset of the n HOST descriptors — the line buffers one after the
 *   other, X Nf uint16 each — and *bytes to their total.  Error -1 for X outside 1..65535, Nf outside 1..4, a total of
 *   2^32 elements or more.
 * hhsr_ljpeg_decode: one launch decodes the n_segs streams into out, uint16 [n_frames][H][W] with rows row_elems and frames
 *   frame_elems ELEMENTS apart (row_elems >= W, frame_elems >= H row_elems: error -1 otherwise; they are pitches, so
 *   nothing between the rows is written).  blob: the streams' entropy-coded bytes, 4-byte aligned, blob_bytes a multiple
 *   of 4 (pad with anything).  Segment i: bytes blob[offset .. offset + length); X samples per line per component, Y
 *   lines, Nf interleaved components, precision P, the scan's predictor, table[c] an index into tables[0 .. n_tables);
 *   it belongs to frame `frame` and covers the rectangle seg_w x seg_h at (x0, y0) — a tile, or a strip of the whole width.
 *     - Bits are taken most significant first; FF 00 is the data byte FF; FF followed by anything else, or the end of the
 *       segment's bytes, ends the data: behind it the reader supplies zero bits, and a segment that consumed one has
 *       status HHSR_LJPEG_TRUNCATED.  The dwords that hold the segment's first and last byte are read whole (they may
 *       hold a neighbour's bytes, never bytes outside the blob).
 *     - Each of the X Y Nf samples: a Huffman code gives SSSS; no code of up to 16 bits in the table ends the segment with
 *       HHSR_LJPEG_BAD_CODE (what was stored before stays).  SSSS = 0: difference 0; 16: 32768, no further bits;
 *       otherwise the next SSSS bits v, v - 2^SSSS + 1 when v < 2^(SSSS-1).  sample = (prediction + difference) mod 2^16.
 *     - Prediction, per component, from Ra (left), Rb (above), Rc (above left) in the JPEG's own X x Y geometry:
 *       2^(P-1) for the first sample, Ra on the rest of the first line, Rb in the first column, else predictor 1 Ra, 2 Rb,
 *       3 Rc, 4 Ra+Rb-Rc, 5 Ra+((Rb-Rc)>>1), 6 Rb+((Ra-Rc)>>1), 7 (Ra+Rb)>>1.  The line above lives in
 *       workspace[line_offset .. line_offset + X Nf), not in out.
 *     - Sample k of the stream (line by line, components interleaved) goes FLAT into the segment: row k / seg_w, column
 *       k % seg_w, as LibRaw and dcraw place it — so a 256-wide CFA tile coded as X = 128, Nf = 2 lands as it should.
 *       It is stored at out[frame][y0 + row][x0 + column] when row < seg_h and the position is inside H x W; every other
 *       sample is decoded and not stored.
 *     - status[i] (DEVICE int32[n_segs]): HHSR_LJPEG_OK, _TRUNCATED, _BAD_CODE, or _BAD_SEGMENT for a descriptor that is
 *       refused before anything is read or written: X or Y outside 1..65535, Nf outside 1..4, X Y Nf > 2^28, P outside
 *       2..16, predictor outside 1..7, bytes outside the blob, frame outside 0..n_frames-1, x0 or y0 < 0, seg_w or seg_h
 *       < 1, a line buffer outside the workspace, a table index outside 0..n_tables-1.
 *   The loop count X Y Nf is fixed before decoding; no input makes a segment read or write outside the ranges above.  One
 *   lane decodes one segment (Huffman decoding is serial within a stream); with up to HHSR_LJPEG_LDS_TABLES tables they
 *   are staged in LDS once per workgroup.  No host synchronisation: the call only enqueues on `stream` and can be captured.
 *   Error -1: a null pointer, n_segs, n_tables, n_frames, H or W <= 0, blob misaligned or blob_bytes % 4 != 0, workspace
 *   or out misaligned for uint16, the pitches above.
 * hhsr_ljpeg_decode_host: the same arguments, every pointer HOST memory, the same per-segment function in a plain loop on
 *   the calling thread; no HIP call, no stream. */
#define HHSR_LJPEG_OK 0
#define HHSR_LJPEG_TRUNCATED 1
#define HHSR_LJPEG_BAD_CODE 2
#define HHSR_LJPEG_BAD_SEGMENT 3
#define HHSR_LJPEG_MAX_COMPONENTS 4
#define HHSR_LJPEG_LOOKUP_BITS 8
#define HHSR_LJPEG_LDS_TABLES 16
typedef struct hhsr_ljpeg_info {
    int32_t P, Y, X, Nf, predictor, point_transform;
    int32_t table[4];         /* DHT id of component c */
    int32_t component_id[4];
    int32_t n_values[4];      /* per DHT id; 0: not present */
    uint8_t bits[4][16];
    uint8_t values[4][17];
    uint32_t data_offset, data_length;
} hhsr_ljpeg_info;
typedef struct hhsr_ljpeg_table {
    uint16_t lookup[1 << HHSR_LJPEG_LOOKUP_BITS];
    int32_t maxcode[18];
    int32_t valoff[17];
    uint8_t values[17];
    uint8_t reserved[3];
} hhsr_ljpeg_table;
typedef struct hhsr_ljpeg_segment {
    uint64_t offset;
    uint32_t length;
    uint32_t line_offset;     /* uint16 elements into the workspace: hhsr_ljpeg_workspace sets it */
    int32_t X, Y, Nf, P, predictor;
    int32_t table[4];
    int32_t frame, x0, y0, seg_w, seg_h;
} hhsr_ljpeg_segment;
int hhsr_ljpeg_parse(const uint8_t* stream_bytes, size_t n_bytes, hhsr_ljpeg_info* info);
int hhsr_ljpeg_tables(const uint8_t* bits, const uint8_t* values, int n, hhsr_ljpeg_table* out);
int hhsr_ljpeg_workspace(hhsr_ljpeg_segment* segs, int n, size_t* bytes);
int hhsr_ljpeg_decode(const uint8_t* blob, size_t blob_bytes, const hhsr_ljpeg_segment* segs, int n_segs,
                      const hhsr_ljpeg_table* tables, int n_tables, uint16_t* workspace, size_t workspace_bytes,
                      uint16_t* out, int n_frames, int H, int W, int64_t row_elems, int64_t frame_elems, int32_t* status,
                      void* stream);
int hhsr_ljpeg_decode_host(const uint8_t* blob, size_t blob_bytes, const hhsr_ljpeg_segment* segs, int n_segs,
                           const hhsr_ljpeg_table* tables, int n_tables, uint16_t* workspace, size_t workspace_bytes,
                           uint16_t* out, int n_frames, int H, int W, int64_t row_elems, int64_t frame_elems,
                           int32_t* status);

/* ---- DNG output: lossless JPEG (run_handheld.py: save_as_dng for a `.dng` path, through exiftool, on the host) -------------
 * The finished image's uint16 samples as the tiles of a DNG with Compression 7, coded on the device: what crosses the host
 * link is the file, not its samples.  Unlike the decoder above the encoder is parallel — every prediction comes from the
 * original samples, so the bits of every sample are independent and only their positions need a prefix sum.  Python's
 * utils_dng.py drives the entry points below and dng.py writes the container; csrc/hhsr_ljpeg_enc_core.h is the one
 * implementation of the per-sample rule, compiled for the host and for the kernels; tests/ljpeg_ref.py is its NumPy form.
 *
 *   samples      uint16 [H][W][Nf], rows row_elems ELEMENTS apart (row_elems >= W Nf; nothing between the rows is read),
 *                2-byte aligned (4-byte aligned with an even row_elems: dword loads).  H, W 1..2^30, Nf 1..4, precision P 2..16,
 *                predictor 1..7.  A sample at or above 2^P is reported (below), never undefined behaviour: the rules
 *                work modulo 2^16.
 *   tiles        tile_h x tile_w, each 16..65535 and a multiple of 16, tile_h tile_w Nf <= 2^28 (what the decoder accepts as
 *                one stream); ceil(H / tile_h) x ceil(W / tile_w) of them in row-major order; the padded image holds at most
 *                2^40 samples.  Tile (ty, tx) is one complete stream with X = tile_w, Y = tile_h and Nf interleaved
 *                components of s(y, x) = image(min(ty tile_h + y, H - 1), min(tx tile_w + x, W - 1)): the edge replicates.
 *   a sample     prediction from Ra (left), Rb (above), Rc (above left) OF THE TILE, as in "DNG input" above: 2^(P-1) for the
 *                first sample, Ra on the first line, Rb in the first column, else the predictor's rule.  difference =
 *                (sample - prediction) mod 2^16 as -32767 .. 32768; SSSS = the bits of its magnitude (32768: 16).  Its bits:
 *                the code word of SSSS, then the SSSS low bits of the difference (of difference - 1 when negative), none
 *                for SSSS 0 and 16.
 *   a stream     SOI; SOF3 (P, Y, X, Nf, component ids 1 .. Nf with H = V = 1, Tq 0); one DHT per component, class 0, id =
 *                the component's index, its bits[16] and values; SOS (component c uses table c; the predictor; no point
 *                transform); the samples' bits line by line, most significant first, padded with 1-bits to a byte, every
 *                FF followed by 00; EOI.  No restart interval.  Exactly tests/ljpeg_ref.py: encode(tile, P, predictor,
 *                tables, comp_table = [0 .. Nf-1]).
 *   the result   the streams one after the other, each at an even offset: offsets[i] (uint64 [n_tiles + 1]) is where stream i
 *                starts and offsets[n_tiles] = *length the end; tile_bytes[i] (uint32 [n_tiles]) is the stream's length
 *                from SOI to EOI.  A stream of odd length is followed by one 00 byte, which offsets[i + 1] - offsets[i]
 *                counts and tile_bytes[i] does not.
 *   bounds       a sample costs at most 16 code bits and 15 magnitude bits (SSSS 16 has none) and every byte of the scan may
 *                be an FF that is stuffed: a stream holds at most  h + 2 ceil(31 tile_h tile_w Nf / 8) + 2  bytes, h =
 *                2 + (10 + 3 Nf) + 38 Nf + (8 + 2 Nf) for SOI, SOF3, Nf DHTs of 17 values and SOS, 2 for EOI; one more for
 *                the even offset.  max_bytes = n_tiles times that; it is below 2^32 per tile, which the offsets scan relies on.
 *
 * hhsr_ljpeg_encode_workspace (host only): *scratch_bytes for hhsr_ljpeg_histogram (one partial table of 72 uint64 for each
 *   of at most 1024 workgroups) and hhsr_ljpeg_encode (4 bytes per tile + 8 per 2048 tiles), the larger; *max_bytes.
 * hhsr_ljpeg_histogram: samples DEVICE -> counts DEVICE uint64 [Nf][17], 8-byte aligned, overwritten: how often each SSSS
 *   occurs per component over all tiles, the replicated samples included.  Exact integers, the same for any row_elems,
 *   alignment and order of the workgroups: LDS atomics per workgroup, one partial table each, summed by a second launch; no
 *   atomics on device memory.  *status (DEVICE uint32): HHSR_LJPEG_OK, or HHSR_LJPEG_BAD_SAMPLE when a sample is >= 2^P.
 *   scratch DEVICE, 8-byte aligned.  Two launches.
 * hhsr_ljpeg_huffman (host only, HOST pointers, no HIP call): counts [17] -> bits [16], values [17] (*n_values of them, the
 *   rest 0) by T.81 Annex K.2, figures K.1 to K.4 with the reserved code point (ties: the larger index): zero counts get
 *   no code, no code is longer than 16 bits or all 1-bits.  Error -1 when no count is set or the sum passes 2^62.
 * hhsr_ljpeg_encode: samples DEVICE and the HOST tables bits [Nf][16], values [Nf][17] -> out[0 .. capacity) DEVICE bytes (no
 *   alignment), offsets, tile_bytes and *length (DEVICE; 8-, 4-, 8-byte aligned).  The code words and the streams' fixed
 *   bytes travel as a by-value kernel argument: no copy, no allocation, the call stays capturable, the tables may be freed on
 *   return.  A result longer than capacity is cut there — no byte outside [out, out + capacity) is written — and offsets,
 *   tile_bytes and *length are still those of the whole result.  A category the tables give no code, or a sample >= 2^P:
 *   *length = UINT64_MAX, the bytes unspecified.  The bytes are the same in every run and on every stream.  One workgroup
 *   per tile walks its stream in batches of 2048 samples (csrc/hhsr_ljpeg_enc.hip).  Five launches: sizes, the offsets scan
 *   (three), the write pass.  No host synchronisation.
 * hhsr_ljpeg_encode_host: the same without scratch and stream, every pointer HOST memory: a plain loop on the calling thread
 *   over the same per-sample function, no HIP call, the same bytes.
 * All: error -1 before any HIP call for a null or misaligned pointer, dimensions, P, predictor or tile outside the above,
 *   row_elems < W Nf, a scratch smaller than stated, overlapping buffers, tables that are no prefix code (per component
 *   1..17 distinct values <= 16, Kraft sum <= 1). */
#define HHSR_LJPEG_BAD_SAMPLE 4
int hhsr_ljpeg_encode_workspace(int H, int W, int Nf, int tile_h, int tile_w, size_t* scratch_bytes, size_t* max_bytes);
int hhsr_ljpeg_histogram(const uint16_t* samples, int H, int W, int Nf, int64_t row_elems, int P, int predictor, int tile_h,
                         int tile_w, uint64_t* counts, uint32_t* status, void* scratch, size_t scratch_bytes, void* stream);
int hhsr_ljpeg_huffman(const uint64_t* counts, uint8_t* bits, uint8_t* values, int* n_values);
int hhsr_ljpeg_encode(const uint16_t* samples, int H, int W, int Nf, int64_t row_elems, int P, int predictor, int tile_h,
                      int tile_w, const uint8_t* bits, const uint8_t* values, void* scratch, size_t scratch_bytes,
                      uint8_t* out, size_t capacity, uint64_t* offsets, uint32_t* tile_bytes, uint64_t* length, void* stream);
int hhsr_ljpeg_encode_host(const uint16_t* samples, int H, int W, int Nf, int64_t row_elems, int P, int predictor, int tile_h,
                           int tile_w, const uint8_t* bits, const uint8_t* values, uint8_t* out, size_t capacity,
                           uint64_t* offsets, uint32_t* tile_bytes, uint64_t* length);

/* ---- measurement support ------------------------------------------------------------------------------------------
 * Shader-clock probe: one wave that sleeps for `ticks_100mhz` ticks of the constant 100 MHz counter and stores
 * {shader cycles, 100 MHz ticks} at its start and end into out4 (DEVICE uint64[4]); launched on a side stream around a
 * timed region, (out4[2] - out4[0]) / (out4[3] - out4[1]) x 100 MHz is the clock the kernels next to it ran at
 * (bench.py's "sclk_mhz").  No counterpart in the reference. */
int hhsr_clock_probe(uint64_t* out4, int64_t ticks_100mhz, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HHSR_H */
