// Grey-image low-pass masks and the Gaussian pyramid (reference utils_image.py:82-100, 360-391;
// alignment.py:27-37, 74-82).  The masks and the padding are small streaming kernels.  The decimating filter was bound by
// VALU issue while it staged a source tile through LDS with per-element address arithmetic (round 6: 87 % VALU busy); it now
// reads each source row into registers once per wave, keeps the addresses in SGPRs and streams at 4.5 - 4.9 TB/s of the bytes
// it has to move (12 MP levels; profiles/pyramid_rob_staging.txt).
#include "hhsr_common.h"

// ---- low-pass masks --------------------------------------------------------------------------
// kept(u): un-shifted bin u survives the reference's zeroing of the fftshift-ed spectrum
// (rows [:n//4] and [-ceil(n/4):] removed; shifted index i = (u + n//2) mod n).
__device__ __forceinline__ bool lp_kept(int u, int n) {
    int i = u + n / 2;
    if (i >= n) i -= n;
    return i >= n / 4 && i < n - (n + 3) / 4;
}

// The spectrum may have any element strides (rocFFT's real transform returns a transposed layout
// through torch); `xfast` says which dimension is contiguous so that a wave reads consecutive bins.
__global__ void __launch_bounds__(256) k_lowpass_c2c(float2* __restrict__ spec, int H, int W, int64_t sy,
                                                      int64_t sx, int xfast) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const int x = xfast ? a : b, y = xfast ? b : a;
    if (x >= W || y >= H) return;
    if (!(lp_kept(y, H) && lp_kept(x, W))) spec[y * sy + x * sx] = make_float2(0.f, 0.f);
}

__global__ void __launch_bounds__(256) k_lowpass_r2c(float2* __restrict__ spec, int H, int W, int Wh, int64_t sy,
                                                      int64_t sx, int xfast) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const int x = xfast ? a : b, y = xfast ? b : a;
    if (x >= Wh || y >= H) return;
    const int ny = y == 0 ? 0 : H - y, nx = x == 0 ? 0 : W - x;
    const int m = (int)(lp_kept(y, H) && lp_kept(x, W)) + (int)(lp_kept(ny, H) && lp_kept(nx, W));
    if (m == 2) return;
    float2 v = spec[y * sy + x * sx];
    const float s = 0.5f * (float)m;
    v.x *= s;
    v.y *= s;
    spec[y * sy + x * sx] = v;
}

extern "C" int hhsr_lowpass_mask_c2c(float* spec, int H, int W, int64_t stride_y, int64_t stride_x, void* stream) {
    HHSR_ARG(spec && H > 0 && W > 0 && stride_y > 0 && stride_x > 0);
    const int xfast = stride_x <= stride_y;
    const dim3 grid = xfast ? dim3(hhsr_cdiv(W, 256), H) : dim3(hhsr_cdiv(H, 256), W);
    hipLaunchKernelGGL(k_lowpass_c2c, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float2*>(spec), H, W,
                       stride_y, stride_x, xfast);
    HHSR_LAUNCHED();
}

extern "C" int hhsr_lowpass_mask_r2c(float* spec, int H, int W, int64_t stride_y, int64_t stride_x, void* stream) {
    HHSR_ARG(spec && H > 0 && W > 0 && stride_y > 0 && stride_x > 0);
    const int Wh = W / 2 + 1;
    const int xfast = stride_x <= stride_y;
    const dim3 grid = xfast ? dim3(hhsr_cdiv(Wh, 256), H) : dim3(hhsr_cdiv(H, 256), Wh);
    hipLaunchKernelGGL(k_lowpass_r2c, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float2*>(spec), H, W,
                       Wh, stride_y, stride_x, xfast);
    HHSR_LAUNCHED();
}

// ---- circular padding ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pad_circular(const float* __restrict__ src, int H, int W, int sp,
                                                       float* __restrict__ dst, int Hp, int Wp, int dp) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= Wp) return;
    dst[(size_t)y * dp + x] = src[(size_t)(y % H) * sp + (x % W)];
}

extern "C" int hhsr_pad_circular(const float* src, int H, int W, int src_pitch, float* dst, int Hp, int Wp,
                                 int dst_pitch, void* stream) {
    HHSR_ARG(src && dst && H > 0 && W > 0 && Hp >= H && Wp >= W && src_pitch >= W && dst_pitch >= Wp);
    hipLaunchKernelGGL(k_pad_circular, dim3(hhsr_cdiv(Wp, 256), Hp), dim3(256), 0, (hipStream_t)stream, src, H, W,
                       src_pitch, dst, Hp, Wp, dst_pitch);
    HHSR_LAUNCHED();
}

// ---- separable Gaussian + decimation ------------------------------------------------------------
struct Taps {
    float g[HHSR_MAX_TAPS];
};

// out[y][x] = sum_j g[j] * (sum_i g[i] * src[f*y+i][f*x+j]): rows first, then columns, both in float32 in
// tap order — the association of the reference's two chained valid conv2d calls.  F and the tap count
// NT = 4F+1 are compile-time so that the loads are issued back to back and the tap loops unroll.
//
// The taps are 58 VALU instructions per output at factor 2; the way to the operands is kept out of the vector pipe (it was
// two thirds of the 168 per output of the kernel that staged a 39 x 71 source tile through LDS):
//   pass 1 (rows), straight from global memory: wave w owns the NV intermediate rows w NV .. w NV + NV - 1 of the tile, a
//     lane 4 source columns.  A thread loads the (NV - 1) F + NT source rows under them once into registers and forms its
//     NV x 4 sums from that window; the row base is wave-uniform (SGPRs), the lane offset one 32-bit register.  VEC (pitch
//     and pointers on the 16-byte grid) and an interior tile — the whole footprint inside the image: lane l holds the
//     columns 4 l .. 4 l + 3 as one 16-byte load per row, no clamp.  Otherwise dwords, lane l holding the columns l + 64 q
//     (coalesced), with the column clamped once per thread and the row clamp in SGPRs, both only on the tiles that reach
//     the right or bottom edge (a clamped operand only feeds outputs past h2 x w2, which are not stored).
//   pass 2 (columns), from the intermediate rows in LDS: wave = row, lane = 4 source columns again, that is the 4 / F
//     adjacent outputs over them; their (4 / F - 1) F + NT operands are one run that starts on the 16-byte grid and is read
//     as ds_read_b128 (conflict-free; as 8-byte reads the compiler pairs them into ds_read2_b64, at a quarter of the rate).
// No division or modulo per element, no 64-bit lane arithmetic: every global address is an SGPR base plus a 32-bit lane offset.
template <int F>
struct GdTile {
    static constexpr int NT = 4 * F + 1;
    static constexpr int TX = F == 2 ? 120 : 60;  // outputs per tile row: the F TX + 3 F + 1 source columns fit 64 lanes x 4
    static constexpr int NV = F == 2 ? 4 : 2;     // intermediate rows per wave (the window is 4 NR registers)
    static constexpr int TY = 4 * NV;             // four waves
    static constexpr int IW = (TX - 1) * F + NT, IH = (TY - 1) * F + NT;  // source footprint
    static constexpr int NL = (IW + 3) / 4;       // lanes that hold columns
    static constexpr int PW = 4 * NL;             // columns loaded = pitch of the intermediate rows
    static constexpr int NR = (NV - 1) * F + NT;  // source rows per thread
    static constexpr int PO = 4 / F;              // pass 2: outputs per thread,
    static constexpr int NE = (PO - 1) * F + NT;  //         operands of a thread
    static_assert(PW <= 256 && (TX * F) % 4 == 0 && TX % PO == 0 && TX / PO <= 64 && NE % 4 != 0, "tile");
};

struct GdFrames {  // blockIdx.z = frame of the batch
    const float* src[HHSR_MAX_BATCH];
    float* dst[HHSR_MAX_BATCH];
};

typedef float gd_f4 __attribute__((ext_vector_type(4)));

// A wave-uniform pointer, kept in SGPRs: the load that adds a 32-bit lane offset to it takes the scalar-base form and no
// 64-bit vector addition (left to itself the compiler adds the lane offset to the frame pointer first and walks the rows
// with one 64-bit VALU addition per load).
typedef const __attribute__((address_space(1))) char* gd_gptr;  // (global, so that the loads stay global_load_*)
__device__ __forceinline__ gd_gptr gd_uniform(const float* p) {
    gd_gptr g = (gd_gptr)p;
    asm volatile("" : "+s"(g));
    return g;
}

typedef __attribute__((address_space(1))) char* gd_wptr;
__device__ __forceinline__ gd_wptr gd_uniform_w(float* p) {
    gd_wptr g = (gd_wptr)p;
    asm volatile("" : "+s"(g));
    return g;
}

// pass 1 of a wave: the NV intermediate rows whose first source row is ry0, into tmp[NV][PW]
template <int F, bool VEC>
__device__ __forceinline__ void gd_rows(const float* __restrict__ src, int H, int W, int sp, int ix0, int ry0, bool interior,
                                        int lane, const Taps& taps, float (*tmp)[GdTile<F>::PW]) {
    using T = GdTile<F>;
    float v[T::NR][4];
    if constexpr (VEC) {
        const unsigned lo = 16u * (unsigned)min(lane, T::NL - 1);  // (lanes past NL load a copy and store nothing)
#pragma unroll
        for (int k = 0; k < T::NR; ++k) {
            const gd_gptr rp = gd_uniform(src + (size_t)(ry0 + k) * sp + ix0);
            const gd_f4 t = *(const __attribute__((address_space(1))) gd_f4*)(rp + lo);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[k][q] = t[q];
        }
    } else {
        unsigned lo[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = min(lane + 64 * q, T::PW - 1);
            lo[q] = 4u * (unsigned)(interior ? ix0 + c : min(ix0 + c, W - 1));
        }
#pragma unroll
        for (int k = 0; k < T::NR; ++k) {
            const int y = interior ? ry0 + k : min(ry0 + k, H - 1);
            const gd_gptr rp = gd_uniform(src + (size_t)y * sp);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[k][q] = *(const __attribute__((address_space(1))) float*)(rp + lo[q]);
        }
    }
    float a[T::NV][4];
#pragma unroll
    for (int m = 0; m < T::NV; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < T::NT; ++i) acc += taps.g[i] * v[F * m + i][q];
            a[m][q] = acc;
        }
    if constexpr (VEC) {
        if (lane < T::NL)
#pragma unroll
            for (int m = 0; m < T::NV; ++m) {
                gd_f4 t;
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] = a[m][q];
                *reinterpret_cast<gd_f4*>(&tmp[m][4 * lane]) = t;
            }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (lane + 64 * q < T::PW)
#pragma unroll
                for (int m = 0; m < T::NV; ++m) tmp[m][lane + 64 * q] = a[m][q];
    }
}

template <int F>
__global__ void __launch_bounds__(256) k_gauss_decimate(GdFrames fr, int H, int W, int sp, int h2, int w2, int dp,
                                                         int vec, Taps taps) {
    using T = GdTile<F>;
    __shared__ __attribute__((aligned(16))) float s_tmp[T::TY][T::PW];
    const float* __restrict__ src = fr.src[blockIdx.z];
    float* __restrict__ dst = fr.dst[blockIdx.z];
    const int bid = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);  // bands of tile rows per XCD
    const int ox0 = (bid % gridDim.x) * T::TX, oy0 = (bid / gridDim.x) * T::TY;
    const int ix0 = ox0 * F, iy0 = oy0 * F;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool interior = ix0 + T::PW <= W && iy0 + T::IH <= H;  // per workgroup
    const int ry0 = iy0 + wv * T::NV * F;                         // first source row of the wave
    if (vec && interior)
        gd_rows<F, true>(src, H, W, sp, ix0, ry0, true, lane, taps, &s_tmp[wv * T::NV]);
    else
        gd_rows<F, false>(src, H, W, sp, ix0, ry0, interior, lane, taps, &s_tmp[wv * T::NV]);
    __syncthreads();
    if (lane >= T::TX / T::PO) return;
    const int ox = ox0 + T::PO * lane;
#pragma unroll
    for (int p = 0; p < T::NV; ++p) {
        const int r = wv + 4 * p, oy = oy0 + r;
        if (oy >= h2) break;  // (per wave)
        float t[T::NE + 3];
#pragma unroll
        for (int j = 0; j < T::NE / 4; ++j) {
            const gd_f4 u = *reinterpret_cast<const gd_f4*>(&s_tmp[r][4 * lane + 4 * j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) t[4 * j + e] = u[e];
        }
#pragma unroll
        for (int j = T::NE / 4 * 4; j < T::NE; ++j) t[j] = s_tmp[r][4 * lane + j];
        gd_wptr rp = gd_uniform_w(dst + (size_t)oy * dp + ox0);
#pragma unroll
        for (int e = 0; e < T::PO; ++e) {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < T::NT; ++j) acc += taps.g[j] * t[e * F + j];
            if (ox + e < w2) *(__attribute__((address_space(1))) float*)(rp + 4u * (unsigned)(T::PO * lane + e)) = acc;
        }
    }
}

template <int F>
static void gd_launch(const GdFrames& fr, int nb, int H, int W, int sp, int h2, int w2, int dp, int vec, const Taps& t,
                      hipStream_t stream) {
    const dim3 g(hhsr_cdiv(w2, GdTile<F>::TX), hhsr_cdiv(h2, GdTile<F>::TY), nb);
    hipLaunchKernelGGL(k_gauss_decimate<F>, g, dim3(256), 0, stream, fr, H, W, sp, h2, w2, dp, vec, t);
}

extern "C" int hhsr_gauss_decimate_batch(const float* const* srcs, int n_frames, int H, int W, int src_pitch,
                                         float* const* dsts, int dst_pitch, int factor, const float* taps, int ntaps,
                                         void* stream) {
    HHSR_ARG(srcs && dsts && taps && n_frames >= 0 && H > 0 && W > 0 && src_pitch >= W);
    HHSR_ARG((factor == 2 || factor == 4) && ntaps == 4 * factor + 1);  // the reference's kernels: radius int(2f + 0.5)
    for (int n = 0; n < n_frames; ++n) HHSR_ARG(srcs[n] && dsts[n]);
    const int r = (ntaps - 1) / 2;
    const int h2 = (H - 2 * r) / factor, w2 = (W - 2 * r) / factor;
    HHSR_ARG(h2 > 0 && w2 > 0 && dst_pitch >= w2);
    Taps t;
    for (int i = 0; i < HHSR_MAX_TAPS; ++i) t.g[i] = i < ntaps ? taps[i] : 0.f;
    for (int n0 = 0; n0 < n_frames; n0 += HHSR_MAX_BATCH) {
        const int nb = n_frames - n0 < HHSR_MAX_BATCH ? n_frames - n0 : HHSR_MAX_BATCH;
        GdFrames fr;
        int vec = src_pitch % 4 == 0;  // 16-byte loads: every row of every frame of the launch starts on the 16-byte grid
        for (int k = 0; k < HHSR_MAX_BATCH; ++k) {
            fr.src[k] = srcs[n0 + (k < nb ? k : 0)];
            fr.dst[k] = dsts[n0 + (k < nb ? k : 0)];
            vec = vec && ((uintptr_t)fr.src[k] & 15) == 0;
        }
        if (factor == 2)
            gd_launch<2>(fr, nb, H, W, src_pitch, h2, w2, dst_pitch, vec, t, (hipStream_t)stream);
        else
            gd_launch<4>(fr, nb, H, W, src_pitch, h2, w2, dst_pitch, vec, t, (hipStream_t)stream);
    }
    HHSR_LAUNCHED();
}

extern "C" int hhsr_gauss_decimate(const float* src, int H, int W, int src_pitch, float* dst, int dst_pitch,
                                   int factor, const float* taps, int ntaps, void* stream) {
    HHSR_ARG(src && dst);
    return hhsr_gauss_decimate_batch(&src, 1, H, W, src_pitch, &dst, dst_pitch, factor, taps, ntaps, stream);
}
