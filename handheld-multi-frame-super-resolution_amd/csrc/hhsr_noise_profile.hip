// Noise profile of a burst that brings none (include/hhsr.h "noise profile"): the tile statistic on the device
// (hhsr_noise_profile_hist) and the line fit on the host (hhsr_noise_profile_fit).  No counterpart in the reference, which
// reads (alpha, beta) from the DNG NoiseProfile tag.
#include "hhsr_common.h"

#include <math.h>
#include <string.h>

// ---- the statistic ---------------------------------------------------------------------------------------------------------
// One pass, every byte of every whole 16 x 16 pixel block read once, nothing else read:
//   thread     one quad row of one block: pixel rows 2 y and 2 y + 1, 16 pixels each = 8 quads of the 4 planes, 8 x 16-byte
//              loads where the frame and its row stride are multiples of 16 bytes, 32 dword loads elsewhere (the same values).
//   8 lanes    one block, lane y its quad row y: the rows above and below come from lanes y - 1 and y + 1 by shuffle; the
//              thread adds its row of each plane left to right in float64 (values: all 8 lanes; r r: lanes 1 .. 6).
//   wave       8 blocks side by side; the 8 x 8 row sums of a block go through a wave-private LDS image [8 sums][64 lanes]
//              (sum stride 65 doubles: conflict-free both ways) and lane y adds sum number y of its block top to bottom:
//              lanes 0 .. 3 the value sums of planes 0 .. 3, lanes 4 .. 7 their residual sums, handed to lanes 0 .. 3, which
//              bin the tile and add 1 to the histogram.
//   workgroup  4 waves side by side: NP_SPAN_BLOCKS = 32 blocks, 512 x 16 pixels; grid (ceil(blocks / 32), block rows, frames).
#define NP_WAVES 4
#define NP_WAVE_BLOCKS 8
#define NP_SPAN_BLOCKS (NP_WAVES * NP_WAVE_BLOCKS)
#define NP_SM_STRIDE (HHSR_WAVE + 1)
#define NP_MEAN_BINS 64
#define NP_ENERGY_BINS 1024
#define NP_ENERGY_BASE ((127 - 32) << 5)  // (exponent, 5 mantissa bits) of 2^-32: energy bin 0
#define NP_HIST_BYTES ((size_t)4 * NP_MEAN_BINS * NP_ENERGY_BINS * sizeof(uint32_t))

struct NoiseFrames {
    const uint8_t* p[HHSR_MAX_BATCH];
    float inv_gain[4];
};

__global__ void __launch_bounds__(NP_WAVES* HHSR_WAVE) k_noise_profile(NoiseFrames F, int nbx, size_t row_bytes,
                                                                        uint32_t* __restrict__ hist) {
    __shared__ double sm[NP_WAVES][8 * NP_SM_STRIDE];
    const int lane = threadIdx.x & (HHSR_WAVE - 1), wv = threadIdx.x / HHSR_WAVE;
    const int g = lane >> 3, y = lane & 7;
    const int bx = (blockIdx.x * NP_WAVES + wv) * NP_WAVE_BLOCKS + g;
    const bool live = bx < nbx;  // (the same in the 8 lanes of a block)
    const uint8_t* __restrict__ frame = F.p[blockIdx.z];
    float t[16], b[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = b[k] = 0.0f;  // (a block past the row's end: fails 0 < u)
    if (live) {
        const uint8_t* __restrict__ top = frame + ((size_t)blockIdx.y * 16 + 2 * y) * row_bytes + (size_t)bx * 64;
        const uint8_t* __restrict__ bot = top + row_bytes;
        if (((((uintptr_t)frame) | row_bytes) & 15) == 0) {  // (uniform per frame)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 q = reinterpret_cast<const float4*>(top)[j], r = reinterpret_cast<const float4*>(bot)[j];
                t[4 * j] = q.x, t[4 * j + 1] = q.y, t[4 * j + 2] = q.z, t[4 * j + 3] = q.w;
                b[4 * j] = r.x, b[4 * j + 1] = r.y, b[4 * j + 2] = r.z, b[4 * j + 3] = r.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                t[k] = reinterpret_cast<const float*>(top)[k];
                b[k] = reinterpret_cast<const float*>(bot)[k];
            }
        }
    }
    // u[p][k]: quad k of plane p = (row & 1) * 2 + (col & 1)
    float u[4][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        u[0][k] = t[2 * k] * F.inv_gain[0];
        u[1][k] = t[2 * k + 1] * F.inv_gain[1];
        u[2][k] = b[2 * k] * F.inv_gain[2];
        u[3][k] = b[2 * k + 1] * F.inv_gain[3];
    }
    const bool interior = y >= 1 && y <= 6;
    unsigned long long okmask = 0;
    double* __restrict__ smw = sm[wv];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        bool ok = true;
        double ms = (double)u[p][0];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            ok = ok && (u[p][k] > 0.0f && u[p][k] < 1.0f);  // (NaN fails)
            if (k) ms += (double)u[p][k];
        }
        double ss = 0.0;
#pragma unroll
        for (int k = 1; k <= 6; ++k) {  // every lane shuffles; only the interior rows own a residual
            const float up = __shfl_up(u[p][k], 1, HHSR_WAVE), dn = __shfl_down(u[p][k], 1, HHSR_WAVE);
            const float r = u[p][k] - 0.25f * ((u[p][k - 1] + u[p][k + 1]) + (up + dn));
            const double rr = (double)(r * r);
            ss = k == 1 ? rr : ss + rr;
        }
        smw[p * NP_SM_STRIDE + lane] = ms;
        smw[(4 + p) * NP_SM_STRIDE + lane] = interior ? ss : 0.0;
        const unsigned long long m = __ballot(ok);
        if ((y & 3) == p) okmask = m;
    }
    __syncthreads();
    // lane y: sum number y of its block, rows top to bottom (the first and last rows of a residual sum are 0: x + 0 = x)
    const double* __restrict__ col = smw + y * NP_SM_STRIDE + g * 8;
    double acc = col[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) acc += col[j];
    const double S = __shfl_down(acc, 4, HHSR_WAVE);
    if (live && y < 4 && ((okmask >> (g * 8)) & 0xffull) == 0xffull) {
        const double m = acc / 64.0;
        const float e = (float)(S / 45.0);
        if (e != 0.0f) {
            const int mb = min(NP_MEAN_BINS - 1, (int)(m * 64.0));
            const int eb = clampi((int)(__float_as_uint(e) >> 18) - NP_ENERGY_BASE, 0, NP_ENERGY_BINS - 1);
            atomicAdd(hist + ((size_t)y * NP_MEAN_BINS + mb) * NP_ENERGY_BINS + eb, 1u);
        }
    }
}

extern "C" int hhsr_noise_profile_hist(const void* const* frames, int n_frames, int H, int W, int64_t row_bytes,
                                       const uint8_t* cfa, const float* inv_gain, uint32_t* hist, void* stream) {
    HHSR_ARG(frames && inv_gain && hist);
    HHSR_ARG(n_frames >= 1 && n_frames <= HHSR_MAX_BATCH);
    HHSR_ARG(H > 0 && W > 0 && (H & 1) == 0 && (W & 1) == 0);
    HHSR_ARG(H / 16 <= 65535);  // the grid's y size
    HHSR_ARG(W <= INT32_MAX / 4 && row_bytes >= (int64_t)4 * W && row_bytes % 4 == 0);
    HHSR_ARG(row_bytes <= INT64_MAX / H);  // the byte offset of the last row
    if (cfa)
        for (int k = 0; k < 4; ++k) HHSR_ARG(cfa[k] <= 2);
    for (int n = 0; n < n_frames; ++n) HHSR_ARG(frames[n] != nullptr && ((uintptr_t)frames[n] & 3) == 0);
    HHSR_ARG(((uintptr_t)hist & 3) == 0);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(hist, 0, NP_HIST_BYTES, s);
    if (e != hipSuccess) {
        hhsr_set_error("%s: hipMemsetAsync failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    const int nbx = W / 16, nby = H / 16;
    if (nbx == 0 || nby == 0) return 0;  // a frame smaller than one tile has none
    NoiseFrames F;
    for (int n = 0; n < HHSR_MAX_BATCH; ++n) F.p[n] = (const uint8_t*)frames[n < n_frames ? n : 0];
    for (int k = 0; k < 4; ++k) F.inv_gain[k] = inv_gain[k];
    const dim3 grid((nbx + NP_SPAN_BLOCKS - 1) / NP_SPAN_BLOCKS, nby, n_frames);
    hipLaunchKernelGGL(k_noise_profile, grid, dim3(NP_WAVES * HHSR_WAVE), 0, s, F, nbx, (size_t)row_bytes, hist);
    HHSR_LAUNCHED();
}

// ---- the fit (host only) -----------------------------------------------------------------------------------------------------
static double np_edge(int k) {  // lower edge of energy bin k (k = 1024: the upper edge of the last bin, 1.0)
    const uint32_t bits = (uint32_t)(k + NP_ENERGY_BASE) << 18;
    float f;
    memcpy(&f, &bits, sizeof f);
    return (double)f;
}

// One colour: the planes `mask` (bit p) of hist added; -> (alpha, beta), the number of usable mean bins
static int np_fit_colour(const uint32_t* hist, unsigned mask, int min_tiles, double* alpha, double* beta) {
    double Sw = 0.0, Swx = 0.0, Swy = 0.0, Swxx = 0.0, Swxy = 0.0;
    int used = 0;
    for (int b = 0; b < NP_MEAN_BINS; ++b) {
        uint64_t cnt[NP_ENERGY_BINS], n = 0;
        for (int k = 0; k < NP_ENERGY_BINS; ++k) {
            uint64_t c = 0;
            for (int p = 0; p < 4; ++p)
                if (mask >> p & 1) c += hist[((size_t)p * NP_MEAN_BINS + b) * NP_ENERGY_BINS + k];
            cnt[k] = c;
            n += c;
        }
        if (n == 0 || n < (uint64_t)(min_tiles > 0 ? min_tiles : 0)) continue;
        const double target = 0.5 * (double)n;
        uint64_t cum = 0;
        double y = 0.0;
        for (int k = 0; k < NP_ENERGY_BINS; ++k) {
            const uint64_t prev = cum;
            cum += cnt[k];
            if (cnt[k] && (double)cum >= target) {
                const double lo = np_edge(k), hi = np_edge(k + 1);
                y = lo + (target - (double)prev) / (double)cnt[k] * (hi - lo);
                break;
            }
        }
        const double x = (b + 0.5) / 64.0, w = (double)n / (y * y);
        Sw += w, Swx += w * x, Swy += w * y, Swxx += w * x * x, Swxy += w * x * y;
        ++used;
    }
    if (used < 2) return used;
    const double det = Sw * Swxx - Swx * Swx;
    double a = (Sw * Swxy - Swx * Swy) / det, c = (Swxx * Swy - Swx * Swxy) / det;
    if (c < 0.0) {
        c = 0.0;
        a = Swxy / Swxx;
    } else if (a < 0.0) {
        a = 0.0;
        c = Swy / Sw;
    }
    *alpha = a, *beta = c;
    return used;
}

extern "C" int hhsr_noise_profile_fit(const uint32_t* hist, const uint8_t* cfa, int min_tiles, double* alpha_beta,
                                      int* bins_used) {
    HHSR_ARG(hist && alpha_beta && bins_used);
    HHSR_ARG(min_tiles >= 1);
    if (cfa)
        for (int k = 0; k < 4; ++k) HHSR_ARG(cfa[k] <= 2);
    int bad = -1;
    for (int c = 0; c < 3; ++c) {
        unsigned mask = 0;
        for (int p = 0; p < 4; ++p)
            if (!cfa || cfa[p] == c) mask |= 1u << p;
        alpha_beta[2 * c] = alpha_beta[2 * c + 1] = 0.0;
        bins_used[c] = np_fit_colour(hist, mask, min_tiles, alpha_beta + 2 * c, alpha_beta + 2 * c + 1);
        if (bins_used[c] < 2 && bad < 0) bad = c;
    }
    // (no CFA: the three pairs are one pair, and so is their mean)
    alpha_beta[6] = cfa ? (alpha_beta[0] + alpha_beta[2] + alpha_beta[4]) / 3.0 : alpha_beta[0];
    alpha_beta[7] = cfa ? (alpha_beta[1] + alpha_beta[3] + alpha_beta[5]) / 3.0 : alpha_beta[1];
    if (bad >= 0) {
        hhsr_set_error("%s: colour %d has %d usable mean bins (of at least %d tiles): a line needs 2", __func__, bad,
                       bins_used[bad], min_tiles);
        return -3;
    }
    return 0;
}
