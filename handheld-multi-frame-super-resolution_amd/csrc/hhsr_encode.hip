// Integer output (include/hhsr.h "integer output"): the finished float32 image -> uint8 / uint16 samples, and the
// accumulated-robustness map -> its grey uint8 mask (reference run_handheld.py:132-159, utils_dng.py:208-215, which do
// this on the host with NumPy / skimage / OpenCV after the float32 image crossed the host link).
//
//   q = rint(clip(nan_to_num(x), 0, 1) * M), half to even, M = 255 or 65535       (float32, one multiply, no contraction)
//
// the rule k_post_expose (hhsr_post.hip) already applies to its exposures.  12 B in + 3 or 6 B out per RGB pixel and
// nothing else: HBM bound.  The output is cut into RUNS of contiguous samples — the whole image when it is compact, one
// row each when the rows are padded — and a run into its 16-byte aligned BODY plus a head and a tail of fewer than 16
// bytes each.  A workgroup converts 4096 bytes of the body: every load instruction is 256 consecutive float4 (lane t
// loads float4 k * 256 + t), a lane packs its four samples into one or two dwords, the dwords cross the workgroup
// through LDS (written at stride 1, read back as b128: both conflict-free) and every lane stores the 16 bytes 16 t ..
// 16 t + 15 of the span — loads and stores both contiguous across the wave.  Loading the 64 consecutive bytes a lane's
// 16 output bytes come from would put the lanes of one load instruction 64 bytes apart (what that costs for stores:
// hhsr_io.hip, k_normalize_packed).  Head and tail are stored sample by sample by the run's first workgroup.  Rows of
// 16-bit samples that start on an odd byte (an odd out_row_bytes puts every other row there) are stored byte by byte.
#include "hhsr_common.h"

__device__ __forceinline__ float encode_sample(float x, float M) {
    x = x == x ? x : 0.f;              // nan_to_num: NaN -> 0 (+-inf -> +-FLT_MAX, which the clip treats as it treats +-inf)
    x = fminf(fmaxf(x, 0.f), 1.f);     // clip(0, 1); -0 stays a zero
    return rintf(x * M);               // one float32 multiply, then round half to even: an integer in [0, M]
}

// samples [0, n) of a run -> dst; sample s is src[s * STEP] (STEP 3: channel 0 of an RGB image, `mode: grey`)
template <typename T, int STEP>
__device__ __forceinline__ void encode_run(const float* __restrict__ src, uint8_t* __restrict__ dstb, size_t n,
                                           unsigned tile, unsigned tiles, float M, uint32_t* __restrict__ lds) {
    constexpr int SPL = 16 / (int)sizeof(T);   // samples per lane = per 16-byte store
    constexpr int NL = SPL / 4;                // float4 loads per lane
    const int t = threadIdx.x;
    if constexpr (sizeof(T) == 2) {
        if ((uintptr_t)dstb & 1) {  // (uniform) a row of 16-bit samples on an odd byte (odd out_row_bytes): byte by byte
            const size_t end = tile + 1 == tiles ? n : (size_t)(tile + 1) * (256 * SPL);
            for (size_t s = (size_t)tile * (256 * SPL) + t; s < end; s += 256) {
                const uint32_t q = (uint32_t)encode_sample(src[s * STEP], M);
                dstb[2 * s] = (uint8_t)(q & 0xffu);
                dstb[2 * s + 1] = (uint8_t)(q >> 8);
            }
            return;
        }
    }
    T* __restrict__ dst = reinterpret_cast<T*>(dstb);
    const size_t to_aligned = ((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(T);  // (dst is aligned to its sample size)
    const size_t head = to_aligned < n ? to_aligned : n;
    const size_t nfull = (n - head) / SPL;     // 16-byte pieces of the body
    const size_t tail0 = head + nfull * SPL;   // first sample of the tail
    if (tile == 0) {  // fewer than SPL samples at either end: sample by sample
        if ((size_t)t < head) dst[t] = (T)encode_sample(src[(size_t)t * STEP], M);
        if (t >= 32 && tail0 + (t - 32) < n) dst[tail0 + (t - 32)] = (T)encode_sample(src[(tail0 + (t - 32)) * STEP], M);
    }
    const size_t piece0 = (size_t)tile * 256;  // first 16-byte piece of this workgroup
    if (piece0 >= nfull) return;               // (uniform: only a run without a body, whose single workgroup ends here)
    const size_t s0 = head + piece0 * SPL;     // first sample of the workgroup's span
    const size_t span = (nfull - piece0 < 256 ? nfull - piece0 : 256) * SPL;  // its samples: a multiple of 4
    const float* __restrict__ in = src + s0 * STEP;
    const bool in16 = STEP == 1 && ((uintptr_t)in & 15) == 0;  // (uniform)
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        const int f = k * 256 + t;             // float4 / sample quadruple f of the span
        if ((size_t)f * 4 < span) {
            float4 v;
            if (in16) {
                v = reinterpret_cast<const float4*>(in)[f];
            } else {
                const float* p = in + (size_t)f * 4 * STEP;
                v = make_float4(p[0], p[STEP], p[2 * STEP], p[3 * STEP]);
            }
            const uint32_t a = (uint32_t)encode_sample(v.x, M), b = (uint32_t)encode_sample(v.y, M),
                           c = (uint32_t)encode_sample(v.z, M), d = (uint32_t)encode_sample(v.w, M);
            if constexpr (sizeof(T) == 1) {
                lds[f] = a | (b << 8) | (c << 16) | (d << 24);
            } else {
                // a quadruple is two dwords; dword j of the span sits at lds[j]: the pair (2 f, 2 f + 1) as one b64 write
                reinterpret_cast<uint2*>(lds)[f] = make_uint2(a | (b << 16), c | (d << 16));
            }
        }
    }
    __syncthreads();
    if ((size_t)t * SPL < span)
        *reinterpret_cast<uint4*>(dst + s0 + (size_t)t * SPL) = reinterpret_cast<const uint4*>(lds)[t];
}

// Runs of n samples each, run y at out + y * out_row_bytes, read from image + y * in_row floats; workgroup b converts
// tile b % tiles of run b / tiles.  A compact image is the single run 0 (both strides are passed as 0).
template <typename T, int STEP>
__global__ void __launch_bounds__(256) k_encode(const float* __restrict__ image, uint8_t* __restrict__ out, size_t n,
                                                 size_t in_row, size_t out_row_bytes, unsigned tiles, float M) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[1024];
    const unsigned row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    encode_run<T, STEP>(image + row * in_row, out + row * out_row_bytes, n, tile, tiles, M, lds);
}

extern "C" int hhsr_encode_image(const float* image, int H, int W, int channels, int out_channels, void* out, int bits,
                                 size_t out_row_bytes, void* stream) {
    HHSR_ARG(image != nullptr && out != nullptr);
    HHSR_ARG(H > 0 && W > 0);
    HHSR_ARG(bits == 8 || bits == 16);
    HHSR_ARG(channels == 1 || channels == 3);
    HHSR_ARG(out_channels == channels || out_channels == 1);
    const size_t bps = (size_t)bits / 8, row_samples = (size_t)W * out_channels, need = row_samples * bps;
    HHSR_ARG(out_row_bytes >= need);
    HHSR_ARG(((uintptr_t)image & 3) == 0 && ((uintptr_t)out & (bps - 1)) == 0);
    HHSR_ARG(out_row_bytes <= (SIZE_MAX - need) / (size_t)H);  // the last row's end, without overflow
    HHSR_ARG((uint64_t)H * W <= (UINT64_MAX >> 5));            // ... and the image's, H W 12 bytes
    const uintptr_t i0 = (uintptr_t)image, i1 = i0 + (size_t)H * W * channels * sizeof(float);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)(H - 1) * out_row_bytes + need;
    HHSR_ARG(o1 <= i0 || i1 <= o0);  // out overlapping image
    // the kernel's sample and byte indices are 64-bit; what has to fit 32 bits is the number of workgroups
    const bool compact = out_row_bytes == need;
    const size_t run = compact ? row_samples * H : row_samples, runs = compact ? 1 : (size_t)H;
    const size_t spl = 16 / bps, pieces = run / spl;  // (a head or a tail only ever takes pieces away from the body)
    const size_t tiles = pieces ? (pieces + 255) / 256 : 1;
    HHSR_ARG(tiles * runs <= (size_t)INT32_MAX);
    const float M = bits == 8 ? 255.f : 65535.f;
    const dim3 grid((unsigned)(tiles * runs)), block(256);
    const size_t in_row = compact ? 0 : (size_t)W * channels;
#define HHSR_ENCODE(T, STEP)                                                                                          \
    hipLaunchKernelGGL((k_encode<T, STEP>), grid, block, 0, (hipStream_t)stream, image, (uint8_t*)out, run, in_row,   \
                       compact ? (size_t)0 : out_row_bytes, (unsigned)tiles, M)
    const bool strided = out_channels != channels;
    if (bits == 8) {
        if (strided) HHSR_ENCODE(uint8_t, 3); else HHSR_ENCODE(uint8_t, 1);
    } else {
        if (strided) HHSR_ENCODE(uint16_t, 3); else HHSR_ENCODE(uint16_t, 1);
    }
#undef HHSR_ENCODE
    HHSR_LAUNCHED();
}

// Robustness mask: out[y][x] = q8(acc[min(y ah / mH, ah - 1)][min(x aw / mW, aw - 1)] / n_comp), the float32 division
// first.  A thread makes four pixels of a row and stores them as one dword where the row allows it.
__global__ void __launch_bounds__(256) k_encode_mask(const float* __restrict__ acc, int ah, int aw, float n_comp,
                                                      uint8_t* __restrict__ out, int mH, int mW, size_t out_row_bytes) {
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x0 >= mW || y >= mH) return;
    const int sy = min((int)(((int64_t)y * ah) / mH), ah - 1);
    const float* __restrict__ arow = acc + (size_t)sy * aw;
    uint8_t* __restrict__ orow = out + (size_t)y * out_row_bytes;
    uint32_t q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = min(x0 + k, mW - 1), sx = min((int)(((int64_t)x * aw) / mW), aw - 1);
        q[k] = (uint32_t)encode_sample(arow[sx] / n_comp, 255.f);
    }
    if (x0 + 4 <= mW && ((uintptr_t)(orow + x0) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(orow + x0) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x0 + k < mW) orow[x0 + k] = (uint8_t)q[k];
    }
}

extern "C" int hhsr_encode_mask(const float* acc_r, int ah, int aw, int n_comp, uint8_t* out, int mH, int mW,
                                size_t out_row_bytes, void* stream) {
    HHSR_ARG(acc_r != nullptr && out != nullptr);
    HHSR_ARG(ah > 0 && aw > 0 && mH > 0 && mW > 0);
    HHSR_ARG(n_comp >= 1);
    HHSR_ARG(out_row_bytes >= (size_t)mW);
    HHSR_ARG(((uintptr_t)acc_r & 3) == 0);
    HHSR_ARG(mW <= INT32_MAX - 1024 && (mH + 3) / 4 <= 65535);  // 32-bit x of a row's last workgroup; rows of workgroups in grid.y
    HHSR_ARG(out_row_bytes <= (SIZE_MAX - (size_t)mW) / (size_t)mH);
    const uintptr_t i0 = (uintptr_t)acc_r, i1 = i0 + (size_t)ah * aw * sizeof(float);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)(mH - 1) * out_row_bytes + (size_t)mW;
    HHSR_ARG(o1 <= i0 || i1 <= o0);
    const dim3 grid(hhsr_cdiv(hhsr_cdiv(mW, 4), 64), hhsr_cdiv(mH, 4));
    hipLaunchKernelGGL(k_encode_mask, grid, dim3(256), 0, (hipStream_t)stream, acc_r, ah, aw, (float)n_comp, out, mH, mW,
                       out_row_bytes);
    HHSR_LAUNCHED();
}
