// Burst front end: sensor counts -> the normalised, white-balanced float32 RAW the hot path
// consumes (reference utils_dng.py:149-160, which does this on the host with NumPy after rawpy decoded the DNGs).
//
//   v = (float32(count) - black[c]) / (white - black[c]);  v *= wb[c] / wb[1]      c = CFA colour of the pixel
//
// in the reference's float32 arithmetic (float32 array op Python scalar -> float32): IEEE subtraction, division
// and multiplication, no contraction, so the result is bit-identical to the NumPy expression.  2 B in / 4 B out
// per pixel: HBM bound; each thread converts 8 pixels of one row (one 16-byte load, two 16-byte stores).
#include "hhsr_common.h"

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

// pixels [0, rem) of the chunk at src -> v (v[rem .. 16) are the padding's, whatever that holds); x0 is a multiple of 16:
// even pixels are CFA column 0.  Reads src[0 .. bytes that hold the rem pixels) and nothing else.
template <int BITS, bool BE>
__device__ __forceinline__ void normalize_chunk(const uint8_t* __restrict__ src, int rem, float (&v)[16], float b0, float b1,
                                                float d0, float d1, float g0, float g1) {
    constexpr int NW = BITS / 2, G = BITS == 12 ? 2 : 4, GB = BITS == 12 ? 3 : BITS / 2;
    uint32_t w[NW], p[16];
    if (rem == 16 && ((uintptr_t)src & 3) == 0) {
#pragma unroll
        for (int j = 0; j < NW; ++j) w[j] = reinterpret_cast<const uint32_t*>(src)[j];
    } else {
        const int nb = BE ? (rem * BITS + 7) >> 3 : (rem + G - 1) / G * GB;  // up to the last bit / group that is used
#pragma unroll
        for (int j = 0; j < NW; ++j) w[j] = 0;
#pragma unroll
        for (int i = 0; i < 4 * NW; ++i)
            if (i < nb) w[i >> 2] |= (uint32_t)src[i] << ((i & 3) * 8);
    }
    unpack16<BITS, BE>(w, p);
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
