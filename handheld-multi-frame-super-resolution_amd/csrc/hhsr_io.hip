// Burst front end: sensor counts -> the normalised, white-balanced float32 RAW the hot path
// consumes (reference utils_dng.py:149-160, which does this on the host with NumPy after rawpy decoded the DNGs).
//
//   v = (float32(count) - black[c]) / (white - black[c]);  v *= wb[c] / wb[1]      c = CFA colour of the pixel
//
// in the reference's float32 arithmetic (float32 array op Python scalar -> float32): IEEE subtraction, division
// and multiplication, no contraction, so the result is bit-identical to the NumPy expression.  2 B in / 4 B out
// per pixel: HBM bound; each thread converts 8 pixels of one row (one 16-byte load, two 16-byte stores).
#include "hhsr_common.h"

#include <math.h>

struct NormArgs {
    float black[4], inv_unused, den[4], gain[4];  // per position of the 2x2 CFA cell: (row & 1) * 2 + (col & 1)
};

__global__ void __launch_bounds__(256) k_normalize_u16(const uint16_t* __restrict__ raw, int W, int pitch_in,
                                                        size_t frame_in, float* __restrict__ out, size_t frame_out,
                                                        int H, NormArgs A) {
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 8, y = blockIdx.y, n = blockIdx.z;
    if (x0 >= W) return;
    const uint16_t* __restrict__ src = raw + n * frame_in + (size_t)y * pitch_in + x0;
    float* __restrict__ dst = out + n * frame_out + (size_t)y * W + x0;
    const int r = (y & 1) * 2;
    const float b0 = A.black[r], b1 = A.black[r + 1], d0 = A.den[r], d1 = A.den[r + 1], g0 = A.gain[r],
                g1 = A.gain[r + 1];
    if (x0 + 8 <= W && ((pitch_in | W) & 7) == 0) {
        const uint4 p = *reinterpret_cast<const uint4*>(src);  // 8 counts; x0 is even: even lanes are CFA column 0
        const uint32_t w[4] = {p.x, p.y, p.z, p.w};
        float v[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = ((float)(w[k] & 0xffffu) - b0) / d0 * g0;
            v[2 * k + 1] = ((float)(w[k] >> 16) - b1) / d1 * g1;
        }
        reinterpret_cast<float4*>(dst)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(dst)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        for (int k = 0; k < 8 && x0 + k < W; ++k) {
            const bool odd = k & 1;
            dst[k] = ((float)src[k] - (odd ? b1 : b0)) / (odd ? d1 : d0) * (odd ? g1 : g0);
        }
    }
}

extern "C" int hhsr_normalize_raw_u16(const uint16_t* raw, int n_frames, int H, int W, int pitch,
                                      const uint8_t cfa[4], const double* black_levels, double white_level,
                                      const double* white_balance, float* out, void* stream) {
    HHSR_ARG(raw && cfa && black_levels && white_balance && out);
    HHSR_ARG(n_frames > 0 && H > 0 && W > 0 && pitch >= W && n_frames <= 65535 && H <= 65535);
    HHSR_ARG(((uintptr_t)raw & 15) == 0 && ((uintptr_t)out & 15) == 0);
    HHSR_ARG(white_balance[1] != 0.0);
    NormArgs A;
    A.inv_unused = 0.f;
    for (int k = 0; k < 4; ++k) {
        HHSR_ARG(cfa[k] <= 2);
        const int c = cfa[k];
        HHSR_ARG(white_level != black_levels[c]);
        A.black[k] = (float)black_levels[c];                 // float32(array) - python scalar -> float32 scalar
        A.den[k] = (float)(white_level - black_levels[c]);   // python arithmetic first, then cast
        A.gain[k] = (float)(white_balance[c] / white_balance[1]);
    }
    const dim3 grid(hhsr_cdiv(hhsr_cdiv(W, 8), 256), H, n_frames);
    hipLaunchKernelGGL(k_normalize_u16, grid, dim3(256), 0, (hipStream_t)stream, raw, W, pitch, (size_t)H * pitch, out,
                       (size_t)H * W, H, A);
    HHSR_LAUNCHED();
}

// ---- packed sensor counts (include/hhsr.h: MIPI CSI-2 RAW10/12/14, TIFF/DNG bit streams of 10/12/14 bits) ------------------
// 16 pixels of a row occupy 2 BITS bytes in every layout (4 or 8 MIPI groups; 16 BITS bits of the stream) and start on a
// byte: one thread converts them — BITS / 2 dwords in, four float4 out.  BITS / 8 B in + 4 B out per pixel: HBM bound like
// the uint16 kernel.  The chunks of a row are 20 / 24 / 28 bytes apart, so whether they are dword-aligned is decided by the
// row's start: uniform per workgroup.  Rows that are not, and the last W % 16 pixels of a row, are read byte by byte and
// only as far as the pixels that are stored reach — the same decoding behind it.

// the counts p[0..16) of one chunk given as little-endian dwords w
template <int BITS, bool BE>
__device__ __forceinline__ void unpack16(const uint32_t (&w)[BITS / 2], uint32_t (&p)[16]) {
    constexpr int NW = BITS / 2;
    if constexpr (BE) {  // pixel k: bits [k BITS, (k + 1) BITS) of the stream, counted from the MSB of byte 0
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int j = (k * BITS) >> 5, off = (k * BITS) & 31;
            const uint64_t two = ((uint64_t)__builtin_bswap32(w[j]) << 32) | (j + 1 < NW ? __builtin_bswap32(w[j + 1]) : 0u);
            p[k] = (uint32_t)(two >> (64 - off - BITS)) & ((1u << BITS) - 1);
        }
    } else {  // groups of G pixels: G bytes of high bits, then the pixels' LB low bits, pixel 0 lowest, little-endian
        constexpr int G = BITS == 12 ? 2 : 4, LB = BITS - 8, GB = G + G * LB / 8;
        auto byte = [&](int i) { return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu; };
#pragma unroll
        for (int g = 0; g < 16 / G; ++g) {
            uint32_t low = 0;
#pragma unroll
            for (int i = 0; i < GB - G; ++i) low |= byte(GB * g + G + i) << (8 * i);
#pragma unroll
            for (int i = 0; i < G; ++i) p[G * g + i] = (byte(GB * g + i) << LB) | ((low >> (LB * i)) & ((1u << LB) - 1));
        }
    }
}

// the 16 counts of a whole chunk that starts on a dword: BITS / 2 dword loads
template <int BITS, bool BE>
__device__ __forceinline__ void read_chunk_whole(const uint8_t* __restrict__ src, uint32_t (&p)[16]) {
    uint32_t w[BITS / 2];
#pragma unroll
    for (int j = 0; j < BITS / 2; ++j) w[j] = reinterpret_cast<const uint32_t*>(src)[j];
    unpack16<BITS, BE>(w, p);
}

// counts [0, rem) of the chunk at src -> p (p[rem .. 16) are the padding's, whatever that holds).  Reads
// src[0 .. bytes that hold the rem pixels) and nothing else: dwords where the chunk is whole and starts on one, bytes
// otherwise.  The ONE reader of the packed layouts: the normalisation below and the sharpness score share it.
template <int BITS, bool BE>
__device__ __forceinline__ void read_chunk(const uint8_t* __restrict__ src, int rem, uint32_t (&p)[16]) {
    constexpr int NW = BITS / 2, G = BITS == 12 ? 2 : 4, GB = BITS == 12 ? 3 : BITS / 2;
    if (rem == 16 && ((uintptr_t)src & 3) == 0) {
        read_chunk_whole<BITS, BE>(src, p);
        return;
    }
    uint32_t w[NW];
    const int nb = BE ? (rem * BITS + 7) >> 3 : (rem + G - 1) / G * GB;  // up to the last bit / group that is used
#pragma unroll
    for (int j = 0; j < NW; ++j) w[j] = 0;
#pragma unroll
    for (int i = 0; i < 4 * NW; ++i)
        if (i < nb) w[i >> 2] |= (uint32_t)src[i] << ((i & 3) * 8);
    unpack16<BITS, BE>(w, p);
}

// pixels [0, rem) of the chunk at src -> v (v[rem .. 16) are the padding's, whatever that holds); x0 is a multiple of 16:
// even pixels are CFA column 0.  Reads what read_chunk reads.
template <int BITS, bool BE>
__device__ __forceinline__ void normalize_chunk(const uint8_t* __restrict__ src, int rem, float (&v)[16], float b0, float b1,
                                                float d0, float d1, float g0, float g1) {
    uint32_t p[16];
    read_chunk<BITS, BE>(src, rem, p);
#pragma unroll
    for (int k = 0; k < 16; k += 2) {
        v[k] = ((float)p[k] - b0) / d0 * g0;
        v[k + 1] = ((float)p[k + 1] - b1) / d1 * g1;
    }
}

// One workgroup: 4096 pixels of one row.  With W % 4 == 0 (every row of out 16-byte aligned) the results go through
// LDS: a thread's own four float4 lie 64 bytes apart from its neighbour's — stored directly, every store instruction of a
// wave touches 64 separate 16-byte pieces (measured at 12 MP: 20 us per frame for every layout against 13.8 us of
// k_normalize_u16, profiles/packed_raw_direct_stores.txt; 11.0 - 11.9 us this way, profiles/packed_raw.txt) — so the
// workgroup stores float4 k * 256 + thread instead, contiguous across the wave.  The four float4 of thread t sit at
// 4 t + ((q + t / 4) & 3): 16 consecutive lanes then cover all 64 banks in the 128-bit write as well as in the read.
// Rows of any other width keep the direct stores, pixel by pixel: correct, and slow (include/hhsr.h states both
// conditions of the fast path).
template <int BITS, bool BE>
__global__ void __launch_bounds__(256) k_normalize_packed(const uint8_t* __restrict__ raw, int W, size_t row_bytes,
                                                           size_t frame_bytes, float* __restrict__ out, size_t frame_out,
                                                           NormArgs A) {
    __shared__ float4 tile[1024];
    const int t = threadIdx.x, chunk = blockIdx.x * 256 + t, x0 = chunk * 16, y = blockIdx.y, n = blockIdx.z;
    const int rem = W - x0 < 16 ? W - x0 : 16;  // <= 0: no pixel of this thread's in the row
    float* __restrict__ orow = out + n * frame_out + (size_t)y * W;
    float v[16];
    if (rem > 0) {
        const int r = (y & 1) * 2;
        normalize_chunk<BITS, BE>(raw + n * frame_bytes + y * row_bytes + (size_t)chunk * (2 * BITS), rem, v, A.black[r],
                                  A.black[r + 1], A.den[r], A.den[r + 1], A.gain[r], A.gain[r + 1]);
    }
    if ((W & 3) == 0) {  // (uniform)
        if (rem > 0) {  // (W % 4 == 0: a float4 holds pixels of the row only or padding only)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                tile[4 * t + ((q + (t >> 2)) & 3)] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int f = k * 256 + t, x = blockIdx.x * 4096 + 4 * f;  // float4 f of the workgroup's span: pixels x .. x + 3
            if (x < W) *reinterpret_cast<float4*>(orow + x) = tile[(f & ~3) | (((f & 3) + (f >> 4)) & 3)];
        }
    } else if (rem > 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < rem) orow[x0 + k] = v[k];
    }
}

// bytes of one packed row of W pixels; 0 for a packing that does not exist
static int64_t packed_row_bytes(int W, int packing) {
    const int64_t w = W;
    switch (packing) {
        case HHSR_PACK_MIPI10: return 5 * ((w + 3) / 4);
        case HHSR_PACK_MIPI12: return 3 * ((w + 1) / 2);
        case HHSR_PACK_MIPI14: return 7 * ((w + 3) / 4);
        case HHSR_PACK_BE10: return (w * 10 + 7) / 8;
        case HHSR_PACK_BE12: return (w * 12 + 7) / 8;
        case HHSR_PACK_BE14: return (w * 14 + 7) / 8;
    }
    return 0;
}

extern "C" int hhsr_packed_row_bytes(int W, int packing, int64_t* bytes_out) {
    HHSR_ARG(bytes_out != nullptr);
    HHSR_ARG(W > 0 && packing >= HHSR_PACK_MIPI10 && packing <= HHSR_PACK_BE14);
    *bytes_out = packed_row_bytes(W, packing);
    return 0;
}

extern "C" int hhsr_normalize_raw_packed(const uint8_t* raw, int n_frames, int H, int W, int64_t row_bytes,
                                         int64_t frame_bytes, int packing, const uint8_t cfa[4],
                                         const double* black_levels, double white_level, const double* white_balance,
                                         float* out, void* stream) {
    HHSR_ARG(raw && cfa && black_levels && white_balance && out);
    HHSR_ARG(packing >= HHSR_PACK_MIPI10 && packing <= HHSR_PACK_BE14);
    HHSR_ARG(n_frames > 0 && H > 0 && W > 0 && n_frames <= 65535 && H <= 65535);
    HHSR_ARG(W <= INT32_MAX - 4096);  // the 32-bit pixel indices of a row's last workgroup
    HHSR_ARG(row_bytes >= packed_row_bytes(W, packing));
    HHSR_ARG(n_frames == 1 || frame_bytes / H >= row_bytes);  // frame_bytes >= H row_bytes, without the product
    HHSR_ARG(((uintptr_t)out & 15) == 0);
    HHSR_ARG(white_balance[1] != 0.0);
    NormArgs A;
    A.inv_unused = 0.f;
    for (int k = 0; k < 4; ++k) {
        HHSR_ARG(cfa[k] <= 2);
        const int c = cfa[k];
        HHSR_ARG(white_level != black_levels[c]);
        A.black[k] = (float)black_levels[c];  // the casts of hhsr_normalize_raw_u16
        A.den[k] = (float)(white_level - black_levels[c]);
        A.gain[k] = (float)(white_balance[c] / white_balance[1]);
    }
    const dim3 grid(hhsr_cdiv(hhsr_cdiv(W, 16), 256), H, n_frames);
    const size_t fb = n_frames == 1 ? 0 : (size_t)frame_bytes;
#define HHSR_PACKED(ID, BITS, BE)                                                                                     \
    case ID:                                                                                                          \
        hipLaunchKernelGGL((k_normalize_packed<BITS, BE>), grid, dim3(256), 0, (hipStream_t)stream, raw, W,           \
                           (size_t)row_bytes, fb, out, (size_t)H * W, A);                                             \
        break;
    switch (packing) {
        HHSR_PACKED(HHSR_PACK_MIPI10, 10, false)
        HHSR_PACKED(HHSR_PACK_MIPI12, 12, false)
        HHSR_PACKED(HHSR_PACK_MIPI14, 14, false)
        HHSR_PACKED(HHSR_PACK_BE10, 10, true)
        HHSR_PACKED(HHSR_PACK_BE12, 12, true)
        HHSR_PACKED(HHSR_PACK_BE14, 14, true)
    }
#undef HHSR_PACKED
    HHSR_LAUNCHED();
}

// ---- sharpness score of the candidate reference frames (include/hhsr.h: "reference selection") --------------------------
// One pass over the frames as they lie in memory — float32, uint16 counts or the packed bytes — 4, 2 or 1.25 - 1.75 bytes
// per pixel in, one double per workgroup out: HBM bound.
//
// Tiling (the same for every format, so that the float64 sum has ONE order per (H, W)):
//   unit       16 pixels x 2 rows = SHARP_UNIT_Q (8) quads of one quad row: one thread, one packed chunk per row
//   wave       64 units side by side, of which it OWNS the first SHARP_WAVE_UNITS (63): 504 quads of one quad row.  The quad
//              right of a unit is the neighbour lane's first (one shuffle); lane 63 only supplies that quad to lane 62 — its
//              unit is the next workgroup's lane 0, read here a second time from cache (1 / 63 of the frame).  A wave walks
//              SHARP_BAND (8) quad rows downwards, carrying the green values of the row above in registers, and reads the
//              quad row below its band once more (1 / 8, rows that the wave below reads at about the same time).
//   workgroup  4 waves below each other: SHARP_TILE_QW x SHARP_TILE_QH = 504 x 32 quads (1008 x 64 pixels);
//              at 12 MP 4 x 47 workgroups per frame.
// Where every unit of a wave is whole and every row starts on 16 bytes (packed: a dword) — all of a 4000-pixel row, any
// compact or 16-byte padded frame — the wave's loads are 16-byte vectors (dwords) with no branch around them; any other
// wave (the row's tail, an odd base or stride) takes the path that decides per unit and reads item by item.  Both paths
// add the same terms in the same order.
// A thread adds its terms in float64 in the order (quad row; quad; dx then dy), the wave adds its lanes by the shuffle
// tree below, thread 0 the four waves in ascending order; k_sharpness_sum adds a frame's workgroups: lane l of one wave
// takes every 64th partial from l on in ascending order, then the same tree.
#define SHARP_UNIT_Q 8
#define SHARP_BAND 8
#define SHARP_WAVES 4
#define SHARP_WAVE_UNITS (HHSR_WAVE - 1)
#define SHARP_TILE_QW (SHARP_UNIT_Q * SHARP_WAVE_UNITS)
#define SHARP_TILE_QH (SHARP_BAND * SHARP_WAVES)
#define SHARP_FMT_F32 0
#define SHARP_FMT_U16 (-1)

struct SharpFrames {
    const uint8_t* p[HHSR_MAX_BATCH];
};

// values [0, rem) of unit u of the row at `row` -> v (the rest 0).  16-byte loads (packed: dwords) where the unit is whole
// and starts on 16 bytes (a dword), item by item otherwise: the same values.  WHOLE: the caller has checked both.
template <int FMT, bool WHOLE>
__device__ __forceinline__ void sharp_load(const uint8_t* __restrict__ row, int u, int rem, float (&v)[16]) {
    if constexpr (FMT == SHARP_FMT_F32) {
        const float* __restrict__ src = reinterpret_cast<const float*>(row) + (size_t)u * 16;
        if (WHOLE || (rem == 16 && ((uintptr_t)src & 15) == 0)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 q = reinterpret_cast<const float4*>(src)[j];
                v[4 * j] = q.x, v[4 * j + 1] = q.y, v[4 * j + 2] = q.z, v[4 * j + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = k < rem ? src[k] : 0.0f;
        }
    } else if constexpr (FMT == SHARP_FMT_U16) {
        const uint16_t* __restrict__ src = reinterpret_cast<const uint16_t*>(row) + (size_t)u * 16;
        if (WHOLE || (rem == 16 && ((uintptr_t)src & 15) == 0)) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint4 q = reinterpret_cast<const uint4*>(src)[j];
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[8 * j + 2 * k] = (float)(w[k] & 0xffffu);
                    v[8 * j + 2 * k + 1] = (float)(w[k] >> 16);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = k < rem ? (float)src[k] : 0.0f;
        }
    } else {
        constexpr int BITS = 10 + 2 * ((FMT - 1) % 3);
        constexpr bool BE = FMT >= HHSR_PACK_BE10;
        uint32_t p[16];
        if constexpr (WHOLE) {
            read_chunk_whole<BITS, BE>(row + (size_t)u * (2 * BITS), p);
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = (float)p[k];
        } else {
            read_chunk<BITS, BE>(row + (size_t)u * (2 * BITS), rem, p);
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = k < rem ? (float)p[k] : 0.0f;
        }
    }
}

// green value of quad k of a unit from its two rows.  (a, b): the two CFA positions that are green, a < b, in cell order
// (row & 1) * 2 + (col & 1); a < 0: no CFA, the mean of the four.
__device__ __forceinline__ float sharp_green(const float (&t)[16], const float (&b)[16], int k, int pa, int pb) {
    const float t0 = t[2 * k], t1 = t[2 * k + 1], b0 = b[2 * k], b1 = b[2 * k + 1];
    if (pa < 0) return ((t0 + t1) + (b0 + b1)) * 0.25f;
    const float va = pa == 0 ? t0 : (pa == 1 ? t1 : b0);
    const float vb = pb == 1 ? t1 : (pb == 2 ? b0 : b1);
    return (va + vb) * 0.5f;
}

__device__ __forceinline__ double sharp_wave_sum(double v) {
#pragma unroll
    for (int o = HHSR_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, HHSR_WAVE);
    return v;  // (lane 0 holds the total)
}

// green values of quad row qy for this thread's unit (g[0 .. 8)) and of the quad right of it (g[8]: the neighbour lane's
// first; lane 63 has none and owns no term).  Quads past the row's end are 0 and enter no term.  All 64 lanes of the wave
// call it (the shuffle).
template <int FMT, bool WHOLE>
__device__ __forceinline__ void sharp_row(const uint8_t* __restrict__ frame, size_t row_bytes, int qy, int u, int rem, int pa,
                                          int pb, float (&g)[SHARP_UNIT_Q + 1]) {
    const uint8_t* __restrict__ top = frame + (size_t)(2 * qy) * row_bytes;
    const uint8_t* __restrict__ bot = top + row_bytes;
    float t[16], b[16];
    if (WHOLE || rem > 0) {
        sharp_load<FMT, WHOLE>(top, u, rem, t);
        sharp_load<FMT, WHOLE>(bot, u, rem, b);
#pragma unroll
        for (int k = 0; k < SHARP_UNIT_Q; ++k) g[k] = sharp_green(t, b, k, pa, pb);
    } else {
#pragma unroll
        for (int k = 0; k < SHARP_UNIT_Q; ++k) g[k] = 0.0f;
    }
    g[SHARP_UNIT_Q] = __shfl_down(g[0], 1, HHSR_WAVE);
}

// the terms of one wave's band, quad rows [y0, y0 + SHARP_BAND) of unit u, whose first quad is q0 (>= w: the thread owns no
// term).  The row below is loaded before the row's terms are added; past the last quad row the last one is loaded again
// (from cache) and enters no term, so that the loop has no branch around its loads and they can be issued rows ahead.
template <int FMT, bool WHOLE>
__device__ __forceinline__ double sharp_band(const uint8_t* __restrict__ frame, size_t row_bytes, int h, int w, int y0, int u,
                                             int rem, int q0, int pa, int pb) {
    double acc = 0.0;
    float cur[SHARP_UNIT_Q + 1], nxt[SHARP_UNIT_Q + 1];
    sharp_row<FMT, WHOLE>(frame, row_bytes, y0, u, rem, pa, pb, cur);
    for (int i = 0; i < SHARP_BAND; ++i) {  // (rolled: unrolling by 2 or 8 measured the same or slower, profiles/ref_select.txt)
        const int qy = y0 + i;
        const bool in = qy < h, below = qy + 1 < h;  // (uniform)
        sharp_row<FMT, WHOLE>(frame, row_bytes, below ? qy + 1 : h - 1, u, rem, pa, pb, nxt);
#pragma unroll
        for (int k = 0; k < SHARP_UNIT_Q; ++k) {
            if (in && q0 + k < w - 1) {
                const float d = cur[k + 1] - cur[k];
                acc += (double)(d * d);
            }
            if (below && q0 + k < w) {
                const float d = nxt[k] - cur[k];
                acc += (double)(d * d);
            }
        }
#pragma unroll
        for (int k = 0; k <= SHARP_UNIT_Q; ++k) cur[k] = nxt[k];
    }
    return acc;
}

// grid (tiles along x, tiles along y, frames); part[(frame * gridDim.y + tile_y) * gridDim.x + tile_x]
template <int FMT>
__global__ void __launch_bounds__(SHARP_WAVES* HHSR_WAVE) k_sharpness(SharpFrames F, int H, int W, size_t row_bytes, int pa,
                                                                       int pb, double* __restrict__ part) {
    __shared__ double sm[SHARP_WAVES];
    const int lane = threadIdx.x & (HHSR_WAVE - 1), wv = threadIdx.x / HHSR_WAVE;
    const int h = H >> 1, w = W >> 1;
    const int u0 = blockIdx.x * SHARP_WAVE_UNITS, u = u0 + lane;
    const int rem = W - 16 * u < 16 ? W - 16 * u : 16;          // <= 0: the unit lies past the row's end
    const int q0 = lane < SHARP_WAVE_UNITS ? u * SHARP_UNIT_Q : w;  // lane 63 is the next workgroup's lane 0: no term here
    const int y0 = blockIdx.y * SHARP_TILE_QH + wv * SHARP_BAND;
    const uint8_t* __restrict__ frame = F.p[blockIdx.z];
    double acc = 0.0;
    if (y0 < h) {  // (uniform per wave)
        // every unit of the wave whole and on 16 bytes (packed: a dword): the loads need no branch; lanes past the row's
        // end then load the workgroup's first unit (it exists and is whole) and own no term
        constexpr uintptr_t align = FMT > 0 ? 3 : 15;
        const bool whole = (rem == 16 || rem <= 0) && ((((uintptr_t)frame) | row_bytes) & align) == 0;
        if (__all(whole))
            acc = sharp_band<FMT, true>(frame, row_bytes, h, w, y0, rem > 0 ? u : u0, 16, q0, pa, pb);
        else
            acc = sharp_band<FMT, false>(frame, row_bytes, h, w, y0, u, rem, q0, pa, pb);
    }
    acc = sharp_wave_sum(acc);
    if (lane == 0) sm[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = sm[0];
#pragma unroll
        for (int k = 1; k < SHARP_WAVES; ++k) s += sm[k];
        part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = s;
    }
}

// one wave per frame: its `tiles` partials -> scores[frame]
__global__ void __launch_bounds__(HHSR_WAVE) k_sharpness_sum(const double* __restrict__ part, int tiles,
                                                              double* __restrict__ scores) {
    const double* __restrict__ row = part + (size_t)blockIdx.x * tiles;
    double acc = 0.0;
    for (int i = threadIdx.x; i < tiles; i += HHSR_WAVE) acc += row[i];
    acc = sharp_wave_sum(acc);
    if (threadIdx.x == 0) scores[blockIdx.x] = acc;
}

// workgroups of one frame; 0 where the sizes are refused
static int64_t sharp_tiles(int H, int W, int* tx, int* ty) {
    if (H <= 0 || W <= 0 || (H & 1) || (W & 1)) return 0;
    if (W > INT32_MAX - 2 * 16 * HHSR_WAVE) return 0;        // 16 u of the lanes behind a row's last unit, in 32 bits
    const int64_t x = ((int64_t)(W / 2) + SHARP_TILE_QW - 1) / SHARP_TILE_QW;
    const int64_t y = ((int64_t)(H / 2) + SHARP_TILE_QH - 1) / SHARP_TILE_QH;
    if (y > 65535 || x * y > INT32_MAX) return 0;            // the grid's y size; the partials of a frame as an int
    *tx = (int)x, *ty = (int)y;
    return x * y;
}

extern "C" int hhsr_sharpness_workspace(int H, int W, int n_frames, size_t* bytes) {
    HHSR_ARG(bytes != nullptr);
    HHSR_ARG(n_frames >= 1 && n_frames <= HHSR_MAX_BATCH);
    int tx, ty;
    const int64_t tiles = sharp_tiles(H, W, &tx, &ty);
    HHSR_ARG(tiles > 0);
    *bytes = (size_t)tiles * n_frames * sizeof(double);
    return 0;
}

extern "C" int hhsr_frame_sharpness(const void* const* frames, int n_frames, int H, int W, int64_t row_bytes, int format,
                                    const uint8_t* cfa, void* workspace, size_t workspace_bytes, double* scores,
                                    void* stream) {
    HHSR_ARG(frames && workspace && scores);
    HHSR_ARG(n_frames >= 1 && n_frames <= HHSR_MAX_BATCH);
    int tx, ty;
    const int64_t tiles = sharp_tiles(H, W, &tx, &ty);
    HHSR_ARG(tiles > 0);
    int pa = -1, pb = -1;
    if (cfa) {
        int greens = 0;
        for (int k = 0; k < 4; ++k) {
            HHSR_ARG(cfa[k] <= 2);
            if (cfa[k] == 1) {
                (greens == 0 ? pa : pb) = k;
                ++greens;
            }
        }
        HHSR_ARG(greens == 2);
    }
    HHSR_ARG(format == SHARP_FMT_F32 || format == SHARP_FMT_U16 || (format >= HHSR_PACK_MIPI10 && format <= HHSR_PACK_BE14));
    const int item = format == SHARP_FMT_F32 ? 4 : (format == SHARP_FMT_U16 ? 2 : 1);
    const int64_t need = format > 0 ? packed_row_bytes(W, format) : (int64_t)item * W;
    HHSR_ARG(row_bytes >= need && row_bytes % item == 0);
    HHSR_ARG(row_bytes <= INT64_MAX / H);  // the byte offset of the last row
    for (int n = 0; n < n_frames; ++n) HHSR_ARG(frames[n] != nullptr && ((uintptr_t)frames[n] & (item - 1)) == 0);
    HHSR_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)scores & 7) == 0);
    HHSR_ARG(workspace_bytes / sizeof(double) / n_frames >= (size_t)tiles);
    SharpFrames F;
    for (int n = 0; n < HHSR_MAX_BATCH; ++n) F.p[n] = (const uint8_t*)frames[n < n_frames ? n : 0];
    const dim3 grid(tx, ty, n_frames);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
#define HHSR_SHARP(ID)                                                                                                \
    case ID:                                                                                                          \
        hipLaunchKernelGGL((k_sharpness<ID>), grid, dim3(SHARP_WAVES* HHSR_WAVE), 0, s, F, H, W, (size_t)row_bytes, pa, \
                           pb, part);                                                                                 \
        break;
    switch (format) {
        HHSR_SHARP(SHARP_FMT_F32)
        HHSR_SHARP(SHARP_FMT_U16)
        HHSR_SHARP(HHSR_PACK_MIPI10)
        HHSR_SHARP(HHSR_PACK_MIPI12)
        HHSR_SHARP(HHSR_PACK_MIPI14)
        HHSR_SHARP(HHSR_PACK_BE10)
        HHSR_SHARP(HHSR_PACK_BE12)
        HHSR_SHARP(HHSR_PACK_BE14)
    }
#undef HHSR_SHARP
    hipLaunchKernelGGL(k_sharpness_sum, dim3(n_frames), dim3(HHSR_WAVE), 0, s, (const double*)part, (int)tiles, scores);
    HHSR_LAUNCHED();
}

// ---- white balance of a burst that brings none (include/hhsr.h: "white balance") -------------------------------------------
// The statistic on the device (hhsr_white_balance_hist), the fit on the host (hhsr_white_balance_fit).  No counterpart in
// the reference, which takes rawpy's camera_whitebalance.  One pass over the counts as they lie in memory, every byte of
// every whole 16 x 16 pixel tile read once, nothing else read:
//   thread     one quad row of one tile: pixel rows 2 y and 2 y + 1, 16 pixels each — per row one packed chunk (read_chunk,
//              dwords) or 32 bytes of uint16 (two 16-byte loads where the frame and its row stride are multiples of 16 bytes,
//              count by count elsewhere: the same values).  It adds its 8 counts of each CFA position in integers and notes
//              whether one of them reaches the position's saturation count.
//   8 lanes    one tile, lane y its quad row y: the four integer sums go through three xor shuffles, the saturation flags
//              through one ballot.  Every lane then holds the tile's sums and forms the two bins; lane 0 of the 8 owns them.
//   wave       8 tiles side by side: 256 contiguous bytes of uint16 per row.
//   workgroup  4 waves side by side, WB_ROWS = 2 tile rows below each other: WB_GROUP_TILES = 64 tiles, 512 x 32 pixels;
//              grid (ceil(tiles / 32), ceil(tile rows / 2), frames).  The tiles' bins meet in LDS, equal bins are merged and
//              the first tile of each bin adds their number with ONE vector integer atomic.
// Everything up to the two float32 quotients is integer; the float32 steps are the single operations of hhsr.h, not
// contracted (build.py), so the histogram is a function of the counts alone.
//
// The atomics decided the form.  An atomic add to an address that others add to completes about every 12 ns on this chip
// (measured below: 46750 adds to one address in 536 us), and a frame puts most tiles into few bins.  12 MP, per frame,
// (textured synthetic frame | uniform grey frame: every tile in ONE bin), one frame per call / eight, uint16:
//   one atomic per tile                     38.6 | 536    us  /  32.1 | 531   us
//   equal bins merged per wave (8 tiles)    36.8 |  74.6      /  29.8 |  69.1
//   merged per workgroup of 32 tiles        22.3 |  24.0      /  16.4 |  18.3
//   merged per workgroup, 2 tile rows       17.4 |  17.1      /  10.3 |  10.4    <- kept (loads of both rows in flight)
//   4 tile rows                             22.1 |  18.0      /  10.8 |   7.4
//   8 tile rows                             26.2 |  21.7      /  10.9 |   6.6
// hhsr_frame_sharpness on the same frames: 15.4 - 15.9 / 5.3 us (profiles/white_balance.txt holds every row; mipi10 rows
// give the same picture).
// More rows per workgroup help only the uniform frame in calls of eight and cost the single-frame call, which is what
// process() makes, its parallelism: 94 x 8 workgroups of 2 rows against 24 x 8 of 8.
#define WB_WAVES 4
#define WB_WAVE_TILES 8
#define WB_SPAN_TILES (WB_WAVES * WB_WAVE_TILES)
#define WB_ROWS 2
#define WB_GROUP_TILES (WB_SPAN_TILES * WB_ROWS)
#define WB_BIN_BASE ((127 - 2) << 5)  // (exponent, 5 mantissa bits) of 2^-2: bin 0
#define WB_HIST_BYTES ((size_t)HHSR_WB_BINS * HHSR_WB_BINS * sizeof(uint32_t))

struct WbArgs {
    const uint8_t* p[HHSR_MAX_BATCH];
    int sat[4];                 // per CFA position: a count >= sat drops the tile
    int colour[4];              // per CFA position: 0 R, 1 G, 2 B
    float black[3], den[3];     // per colour: the casts of hhsr_normalize_raw_u16
};

// the 16 counts of tile column bx of the row at `row`.  FAST: the caller has checked that every row starts on 16 bytes
// (packed: on a dword) — vector loads with no branch around them; otherwise count by count (packed: read_chunk decides).
template <int FMT, bool FAST>
__device__ __forceinline__ void wb_load(const uint8_t* __restrict__ row, int bx, uint32_t (&p)[16]) {
    if constexpr (FMT == SHARP_FMT_U16) {
        const uint16_t* __restrict__ src = reinterpret_cast<const uint16_t*>(row) + (size_t)bx * 16;
        if constexpr (FAST) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint4 q = reinterpret_cast<const uint4*>(src)[j];
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    p[8 * j + 2 * k] = w[k] & 0xffffu;
                    p[8 * j + 2 * k + 1] = w[k] >> 16;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) p[k] = src[k];
        }
    } else {
        constexpr int BITS = 10 + 2 * ((FMT - 1) % 3);
        constexpr bool BE = FMT >= HHSR_PACK_BE10;
        if constexpr (FAST)
            read_chunk_whole<BITS, BE>(row + (size_t)bx * (2 * BITS), p);
        else
            read_chunk<BITS, BE>(row + (size_t)bx * (2 * BITS), 16, p);
    }
}

// bin u * 192 + v of tile (ty, bx), or -1 for a tile that is dropped or, with `live` false, not there: (ty, bx) is then any
// tile that exists, read from cache and thrown away, so that the loads have no branch around them and those of a
// workgroup's WB_ROWS tile rows can all be in flight at once.  Valid in all 8 lanes of the tile; all 64 lanes of the wave
// call it (the shuffles).
template <int FMT, bool FAST>
__device__ __forceinline__ int wb_tile_bin(const WbArgs& A, const uint8_t* __restrict__ frame, size_t row_bytes, int ty, int bx,
                                           bool live, int g, int y) {
    const uint8_t* __restrict__ top = frame + ((size_t)ty * 16 + 2 * y) * row_bytes;
    uint32_t t[16], b[16];
    wb_load<FMT, FAST>(top, bx, t);
    wb_load<FMT, FAST>(top + row_bytes, bx, b);
    int s[4] = {0, 0, 0, 0};
    uint32_t mx[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s[0] += (int)t[2 * k], s[1] += (int)t[2 * k + 1], s[2] += (int)b[2 * k], s[3] += (int)b[2 * k + 1];
        mx[0] = max(mx[0], t[2 * k]), mx[1] = max(mx[1], t[2 * k + 1]);
        mx[2] = max(mx[2], b[2 * k]), mx[3] = max(mx[3], b[2 * k + 1]);
    }
    bool clipped = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) clipped = clipped || (int)mx[q] >= A.sat[q];
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] += __shfl_xor(s[q], o, HHSR_WAVE);
    }
    const bool tile_clipped = ((__ballot(clipped) >> (g * 8)) & 0xffull) != 0;
    int S[3] = {0, 0, 0};  // per colour: 64 counts of R and B, 128 of G, < 2^24
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int c = 0; c < 3; ++c) S[c] += A.colour[q] == c ? s[q] : 0;
    }
    const float mr = ((float)S[0] / 64.0f - A.black[0]) / A.den[0];
    const float mg = ((float)S[1] / 128.0f - A.black[1]) / A.den[1];
    const float mb = ((float)S[2] / 64.0f - A.black[2]) / A.den[2];
    const float lo = 1.0f / 64.0f;
    if (live && !tile_clipped && mr >= lo && mg >= lo && mb >= lo) {  // (NaN fails)
        const int u = (int)(__float_as_uint(mg / mr) >> 18) - WB_BIN_BASE;
        const int v = (int)(__float_as_uint(mg / mb) >> 18) - WB_BIN_BASE;
        if (u >= 0 && u < HHSR_WB_BINS && v >= 0 && v < HHSR_WB_BINS) return u * HHSR_WB_BINS + v;
    }
    return -1;
}

// the bins of the workgroup's tiles -> sb[tile row][tile column]
template <int FMT, bool FAST>
__device__ __forceinline__ void wb_rows(const WbArgs& A, const uint8_t* __restrict__ frame, size_t row_bytes, int nbx, int nby,
                                        int* __restrict__ sb) {
    const int lane = threadIdx.x & (HHSR_WAVE - 1), wv = threadIdx.x / HHSR_WAVE;
    const int g = lane >> 3, y = lane & 7;
    const int bx = (blockIdx.x * WB_WAVES + wv) * WB_WAVE_TILES + g;
    constexpr int rows = WB_ROWS, unrolled = FAST ? rows : 1;  // (the slow path is long code: kept rolled)
#pragma unroll unrolled
    for (int r = 0; r < rows; ++r) {
        const int ty = blockIdx.y * WB_ROWS + r;  // (uniform)
        const bool live = bx < nbx && ty < nby;   // (the same in the 8 lanes of a tile)
        const int bin = wb_tile_bin<FMT, FAST>(A, frame, row_bytes, min(ty, nby - 1), min(bx, nbx - 1), live, g, y);
        if (y == 0) sb[r * WB_SPAN_TILES + wv * WB_WAVE_TILES + g] = bin;
    }
}

template <int FMT>
__global__ void __launch_bounds__(WB_WAVES* HHSR_WAVE) k_white_balance(WbArgs A, int nbx, int nby, size_t row_bytes,
                                                                        uint32_t* __restrict__ hist) {
    __shared__ __attribute__((aligned(16))) int sb[WB_GROUP_TILES];
    const uint8_t* __restrict__ frame = A.p[blockIdx.z];
    constexpr uintptr_t align = FMT > 0 ? 3 : 15;
    if (((((uintptr_t)frame) | row_bytes) & align) == 0)  // (uniform per frame)
        wb_rows<FMT, true>(A, frame, row_bytes, nbx, nby, sb);
    else
        wb_rows<FMT, false>(A, frame, row_bytes, nbx, nby, sb);
    __syncthreads();
    // equal bins among the workgroup's tiles: the first of them adds their number
    for (int e = threadIdx.x; e < WB_GROUP_TILES; e += WB_WAVES * HHSR_WAVE) {
        const int mine = sb[e];
        unsigned cnt = 0;
        bool first = true;
        for (int j = 0; j < WB_GROUP_TILES; j += 4) {
            const int4 q = *reinterpret_cast<const int4*>(sb + j);  // (the same address in every lane: a broadcast)
            const int bj[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                cnt += bj[k] == mine;
                first = first && !(j + k < e && bj[k] == mine);
            }
        }
        if (mine >= 0 && first) atomicAdd(hist + mine, cnt);
    }
}

extern "C" int hhsr_white_balance_hist(const void* const* frames, int n_frames, int H, int W, int64_t row_bytes, int format,
                                       const uint8_t cfa[4], const double* black_levels, double white_level, uint32_t* hist,
                                       void* stream) {
    HHSR_ARG(frames && cfa && black_levels && hist);
    HHSR_ARG(n_frames >= 1 && n_frames <= HHSR_MAX_BATCH);
    int tx, ty;
    HHSR_ARG(sharp_tiles(H, W, &tx, &ty) > 0);  // the limits of hhsr_frame_sharpness: H, W even and > 0, 32-bit indices
    HHSR_ARG(H / 16 <= 65535);                  // the grid's y size
    HHSR_ARG(format == SHARP_FMT_U16 || (format >= HHSR_PACK_MIPI10 && format <= HHSR_PACK_BE14));
    int count[3] = {0, 0, 0};
    for (int k = 0; k < 4; ++k) {
        HHSR_ARG(cfa[k] <= 2);
        ++count[cfa[k]];
    }
    HHSR_ARG(count[0] == 1 && count[1] == 2 && count[2] == 1);
    const int item = format == SHARP_FMT_U16 ? 2 : 1;
    const int64_t need = format > 0 ? packed_row_bytes(W, format) : (int64_t)item * W;
    HHSR_ARG(row_bytes >= need && row_bytes % item == 0);
    HHSR_ARG(row_bytes <= INT64_MAX / H);  // the byte offset of the last row
    for (int n = 0; n < n_frames; ++n) HHSR_ARG(frames[n] != nullptr && ((uintptr_t)frames[n] & (item - 1)) == 0);
    HHSR_ARG(((uintptr_t)hist & 3) == 0);
    WbArgs A;
    for (int c = 0; c < 3; ++c) {
        HHSR_ARG(white_level > black_levels[c]);
        A.black[c] = (float)black_levels[c];  // the casts of hhsr_normalize_raw_u16
        A.den[c] = (float)(white_level - black_levels[c]);
    }
    for (int k = 0; k < 4; ++k) {
        const int c = cfa[k];
        const double sat = ceil(black_levels[c] + 15.0 / 16.0 * (white_level - black_levels[c]));
        A.colour[k] = c;
        A.sat[k] = sat >= 65536.0 ? 65536 : (sat > 0.0 ? (int)sat : 0);  // (a count is at most 65535; NaN: 0, every tile dropped)
    }
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(hist, 0, WB_HIST_BYTES, s);
    if (e != hipSuccess) {
        hhsr_set_error("%s: hipMemsetAsync failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    const int nbx = W / 16, nby = H / 16;
    if (nbx == 0 || nby == 0) return 0;  // a frame smaller than one tile has none
    for (int n = 0; n < HHSR_MAX_BATCH; ++n) A.p[n] = (const uint8_t*)frames[n < n_frames ? n : 0];
    const dim3 grid((nbx + WB_SPAN_TILES - 1) / WB_SPAN_TILES, (nby + WB_ROWS - 1) / WB_ROWS, n_frames);
#define HHSR_WB(ID)                                                                                                   \
    case ID:                                                                                                          \
        hipLaunchKernelGGL((k_white_balance<ID>), grid, dim3(WB_WAVES* HHSR_WAVE), 0, s, A, nbx, nby, (size_t)row_bytes, hist); \
        break;
    switch (format) {
        HHSR_WB(SHARP_FMT_U16)
        HHSR_WB(HHSR_PACK_MIPI10)
        HHSR_WB(HHSR_PACK_MIPI12)
        HHSR_WB(HHSR_PACK_MIPI14)
        HHSR_WB(HHSR_PACK_BE10)
        HHSR_WB(HHSR_PACK_BE12)
        HHSR_WB(HHSR_PACK_BE14)
    }
#undef HHSR_WB
    HHSR_LAUNCHED();
}

// the fit (host only): centre of bin k in log2 units
static double wb_centre(int k) { return log2(ldexp(1.0 + ((k & 31) + 0.5) / 32.0, (k >> 5) - 2)); }

extern "C" int hhsr_white_balance_fit(const uint32_t* hist, int min_tiles, double white_balance[3], int64_t tiles[2]) {
    HHSR_ARG(hist && white_balance && tiles);
    HHSR_ARG(min_tiles >= 1);
    double centre[HHSR_WB_BINS];
    for (int k = 0; k < HHSR_WB_BINS; ++k) centre[k] = wb_centre(k);
    // the count-weighted centroid of the bins within `radius` of (cu, cv) (radius < 0: of all bins), rows then columns
    auto centroid = [&](double cu, double cv, double radius, double* ou, double* ov) {
        double su = 0.0, sv = 0.0;
        int64_t n = 0;
        for (int u = 0; u < HHSR_WB_BINS; ++u)
            for (int v = 0; v < HHSR_WB_BINS; ++v) {
                const uint32_t c = hist[u * HHSR_WB_BINS + v];
                if (c == 0) continue;
                if (radius >= 0.0) {
                    const double du = centre[u] - cu, dv = centre[v] - cv;
                    if (!(du * du + dv * dv <= radius * radius)) continue;
                }
                su += (double)c * centre[u], sv += (double)c * centre[v], n += c;
            }
        if (n > 0) *ou = su / (double)n, *ov = sv / (double)n;
        return n;
    };
    double u = 0.0, v = 0.0;
    const int64_t N = centroid(0.0, 0.0, -1.0, &u, &v);
    tiles[0] = N, tiles[1] = 0;
    white_balance[0] = white_balance[1] = white_balance[2] = 1.0;
    if (N < min_tiles) {
        hhsr_set_error("%s: %lld usable tiles, fewer than min_tiles = %d", __func__, (long long)N, min_tiles);
        return -3;
    }
    for (int it = 0; it < 4; ++it) {
        const int64_t n = centroid(u, v, 0.5, &u, &v);
        tiles[1] = n;
        if (n == 0) break;  // an empty gate: the estimate stays
    }
    white_balance[0] = exp2(u), white_balance[2] = exp2(v);
    return 0;
}

// ---- shader-clock probe (measurement support: bench.py's "sclk_mhz") --------------------------------------------
// ONE wave reads the shader-cycle counter (s_memtime: one tick per shader clock, MI355X_MICROARCH.md "s_memtime tick")
// and the constant 100 MHz counter (s_memrealtime) when it starts, sleeps until `ticks` of the constant counter have
// passed (s_sleep: no issue slots taken from the kernels it runs next to) and reads both again.  Launched on a side
// stream around a timed region it reports the clock the other kernels ACTUALLY ran at: out = {memtime0, realtime0,
// memtime1, realtime1}; sclk = (out[2] - out[0]) / (out[3] - out[1]) x 100 MHz.
__global__ void __launch_bounds__(64) k_clock_probe(unsigned long long* __restrict__ out, long long ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long c0 = __builtin_readcyclecounter(), r0 = wall_clock64();
    unsigned long long r1 = r0;
    while ((long long)(r1 - r0) < ticks) {
        __builtin_amdgcn_s_sleep(127);
        r1 = wall_clock64();
    }
    const unsigned long long c1 = __builtin_readcyclecounter();
    out[0] = c0;
    out[1] = r0;
    out[2] = c1;
    out[3] = r1;
}

extern "C" int hhsr_clock_probe(uint64_t* out4, int64_t ticks_100mhz, void* stream) {
    HHSR_ARG(out4 != nullptr);
    HHSR_ARG(ticks_100mhz >= 0 && ticks_100mhz <= 1000000000LL);  // at most 10 s
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)out4,
                       (long long)ticks_100mhz);
    HHSR_LAUNCHED();
}
