// Noise curves of the robustness noise model (reference fast_monte_carlo.py): the Monte-Carlo estimator as one fused
// kernel + a per-level sum, and the host-side pieces around it (which levels to simulate, interpolation of the rest).
// The stream is stated operation by operation in include/hhsr.h; tests/noise_mc_ref.py is its NumPy form.
#include "hhsr_common.h"

#include <math.h>

#define NMC_THREADS 256
#define NMC_ITEMS (HHSR_NOISE_MC_CHUNK / NMC_THREADS)  // patch pairs per thread
#define NMC_LEVELS 1001                                 // brightness 0, 0.001, ..., 1
static_assert(HHSR_NOISE_MC_CHUNK % NMC_THREADS == 0, "a chunk is a whole number of patch pairs per thread");

// ---- Philox4x32-10 (Salmon et al., SC'11) ---------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t x[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// One Box-Muller pair from two words; precise logf / sincosf (why not the fast intrinsics).
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& z0, float& z1) {
    const float u1 = ((float)(xa >> 8) + 0.5f) * 0x1p-24f;
    const float u2 = ((float)(xb >> 8) + 0.5f) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincosf(6.283185307179586f * u2, &sn, &cs);
    z0 = r * cs;
    z1 = r * sn;
}

// (mean, standard deviation) of one clipped 3 x 3 patch, float32, left to right.
__device__ __forceinline__ void patch_stats(const float* z, float b, float s, float& m, float& sd) {
    float p[9], sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        p[j] = fminf(fmaxf(b + s * z[j], 0.0f), 1.0f);
        sum += p[j];
    }
    m = sum / 9.0f;
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const float d = p[j] - m;
        ss += d * d;
    }
    sd = sqrtf(ss / 9.0f);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = HHSR_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, HHSR_WAVE);
    return v;  // (lane 0 holds the total)
}

// grid (chunks, n_levels): workgroup (c, l) simulates the patch pairs [c CHUNK, (c + 1) CHUNK) of level levels[l] and
// stores their two float64 sums at part[l chunks + c] and part[(n_levels + l) chunks + c].
__global__ __launch_bounds__(NMC_THREADS) void k_noise_mc(const int32_t* __restrict__ levels, int n_levels, float alpha,
                                                          float beta, uint32_t n_patches, uint32_t key0, uint32_t key1,
                                                          double* __restrict__ part) {
    __shared__ double sm[2 * NMC_THREADS / HHSR_WAVE];
    const uint32_t chunks = gridDim.x, chunk = blockIdx.x, l = blockIdx.y;
    const int i = clampi(levels[l], 0, NMC_LEVELS - 1);  // (device memory: the host cannot check the range)
    const float b = (float)((double)i / 1000.0);
    const float s = sqrtf(b * alpha + beta);
    double acc_s = 0.0, acc_d = 0.0;
    for (int it = 0; it < NMC_ITEMS; ++it) {
        const uint32_t p = chunk * HHSR_NOISE_MC_CHUNK + it * NMC_THREADS + threadIdx.x;
        if (p < n_patches) {
            float z[20];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                uint32_t x[4];
                philox4x32_10(p, (uint32_t)i, (uint32_t)k, 0u, key0, key1, x);
                box_muller(x[0], x[1], z[4 * k], z[4 * k + 1]);
                box_muller(x[2], x[3], z[4 * k + 2], z[4 * k + 3]);
            }
            float m1, sd1, m2, sd2;
            patch_stats(z, b, s, m1, sd1);
            patch_stats(z + 9, b, s, m2, sd2);
            acc_s += (double)(0.5f * (sd1 + sd2));
            acc_d += (double)fabsf(m1 - m2);
        }
    }
    acc_s = wave_sum_f64(acc_s);
    acc_d = wave_sum_f64(acc_d);
    const int lane = threadIdx.x & (HHSR_WAVE - 1), w = threadIdx.x / HHSR_WAVE;
    if (lane == 0) {
        sm[2 * w] = acc_s;
        sm[2 * w + 1] = acc_d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = sm[0], td = sm[1];
#pragma unroll
        for (int k = 1; k < NMC_THREADS / HHSR_WAVE; ++k) {
            ts += sm[2 * k];
            td += sm[2 * k + 1];
        }
        part[(size_t)l * chunks + chunk] = ts;
        part[((size_t)n_levels + l) * chunks + chunk] = td;
    }
}

// One thread per (curve, level): its partials in ascending chunk order, then / n_patches.
__global__ __launch_bounds__(NMC_THREADS) void k_noise_mc_sum(const double* __restrict__ part, int n_levels, int chunks,
                                                              double n_patches, double* __restrict__ sigma,
                                                              double* __restrict__ diff) {
    const int t = blockIdx.x * NMC_THREADS + threadIdx.x;
    if (t >= 2 * n_levels) return;
    const double* row = part + (size_t)t * chunks;
    double sum = 0.0;
    for (int c = 0; c < chunks; ++c) sum += row[c];
    const double mean = sum / n_patches;
    if (t < n_levels)
        sigma[t] = mean;
    else
        diff[t - n_levels] = mean;
}

static inline int nmc_chunks(int n_patches) { return (int)(((int64_t)n_patches + HHSR_NOISE_MC_CHUNK - 1) / HHSR_NOISE_MC_CHUNK); }

extern "C" int hhsr_noise_mc_levels(double alpha, double beta, int32_t* levels, int n, int32_t* n_out) {
    HHSR_ARG(n_out);
    HHSR_ARG(isfinite(alpha) && isfinite(beta));
    // get_non_linearity_bound(alpha, beta, tol = 3) and run_fast_MC's index arithmetic, in float64 with its association
    const double t2 = 9.0, n1000 = 1000.0;
    const double xmin = t2 / 2 * (alpha + sqrt(t2 * alpha * alpha + 4 * beta));
    const double B = 2 + t2 * alpha;
    const double xmax = (B - sqrt(B * B - 4 * (1 + t2 * beta))) / 2;
    const double imin_d = ceil(xmin * n1000) + 1, imax_d = floor(xmax * n1000) - 1;
    int imin = NMC_LEVELS - 1, imax = NMC_LEVELS - 1, count = NMC_LEVELS;
    // (negated comparisons: a NaN bound takes the fallback; so does imax > 999 — both where the reference raises)
    const bool fallback = !(imin_d <= n1000) || !(imax_d > imin_d) || !(imin_d >= 0) || !(imax_d <= n1000 - 1);
    if (!fallback) {
        imin = (int)imin_d;
        imax = (int)imax_d;
        count = (imin + 1) + (NMC_LEVELS - imax);
    }
    *n_out = count;
    HHSR_ARG(levels && n >= count);
    if (fallback) {
        for (int i = 0; i < NMC_LEVELS; ++i) levels[i] = i;
        return 0;
    }
    int k = 0;
    for (int i = 0; i <= imin; ++i) levels[k++] = i;
    for (int i = imax; i < NMC_LEVELS; ++i) levels[k++] = i;
    return 0;
}

extern "C" int hhsr_noise_mc_workspace(int n_levels, int n_patches, size_t* bytes) {
    HHSR_ARG(bytes);
    HHSR_ARG(n_levels >= 1 && n_levels <= NMC_LEVELS && n_patches >= 1);
    *bytes = (size_t)2 * n_levels * nmc_chunks(n_patches) * sizeof(double);
    return 0;
}

extern "C" int hhsr_noise_mc(const int32_t* levels, int n_levels, double alpha, double beta, int n_patches, uint64_t seed,
                             double* sigma, double* diff, void* workspace, size_t workspace_bytes, void* stream) {
    HHSR_ARG(levels && sigma && diff && workspace);
    HHSR_ARG(n_levels >= 1 && n_levels <= NMC_LEVELS && n_patches >= 1);
    HHSR_ARG(isfinite(alpha) && isfinite(beta) && alpha >= 0 && beta >= 0);
    HHSR_ARG(((uintptr_t)levels & 3) == 0 && ((uintptr_t)sigma & 7) == 0 && ((uintptr_t)diff & 7) == 0 &&
             ((uintptr_t)workspace & 7) == 0);
    const int chunks = nmc_chunks(n_patches);
    HHSR_ARG(workspace_bytes >= (size_t)2 * n_levels * chunks * sizeof(double));
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(k_noise_mc, dim3(chunks, n_levels), dim3(NMC_THREADS), 0, s, levels, n_levels, (float)alpha,
                       (float)beta, (uint32_t)n_patches, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), part);
    hipLaunchKernelGGL(k_noise_mc_sum, dim3(hhsr_cdiv(2 * n_levels, NMC_THREADS)), dim3(NMC_THREADS), 0, s,
                       (const double*)part, n_levels, chunks, (double)n_patches, sigma, diff);
    HHSR_LAUNCHED();
}

extern "C" int hhsr_noise_curves_fill(const int32_t* levels, int n_levels, const double* sigma, const double* diff,
                                      double* std_curve, double* diff_curve) {
    HHSR_ARG(levels && sigma && diff && std_curve && diff_curve);
    HHSR_ARG(n_levels >= 1 && n_levels <= NMC_LEVELS);
    bool have[NMC_LEVELS] = {};
    for (int k = 0; k < n_levels; ++k) {
        const int i = levels[k];
        if (i < 0 || i >= NMC_LEVELS || have[i]) {
            hhsr_set_error("%s: invalid argument: levels[%d] = %d is outside 0..1000 or given twice", __func__, k, i);
            return -1;
        }
        have[i] = true;
    }
    // the simulated levels are 0..imin and imax..1000: one gap, or none
    int imin = 0, imax = NMC_LEVELS - 1;
    HHSR_ARG(have[0] && have[NMC_LEVELS - 1]);
    while (imin + 1 < NMC_LEVELS && have[imin + 1]) ++imin;
    while (imax - 1 >= 0 && have[imax - 1]) --imax;
    if (imin < NMC_LEVELS - 1) {
        int missing = 0;
        for (int i = 0; i < NMC_LEVELS; ++i) missing += !have[i];
        if (missing != imax - imin - 1) {
            hhsr_set_error("%s: invalid argument: the levels are not 0..imin and imax..1000", __func__);
            return -1;
        }
    }
    for (int k = 0; k < n_levels; ++k) {
        std_curve[levels[k]] = sigma[k];
        diff_curve[levels[k]] = diff[k];
    }
    if (imin == NMC_LEVELS - 1) return 0;  // all 1001 simulated: a copy
    // interp_MC over brightness[imin - 1 .. imax + 1]: sigma^2 and d^2 linear in b between their values at imin and imax,
    // written to imin .. imax (both ends included, as run_fast_MC does)
    const double s_lo = std_curve[imin], s_hi = std_curve[imax], d_lo = diff_curve[imin], d_hi = diff_curve[imax];
    const double b0 = (imin - 1) / 1000.0, b1 = (imax + 1) / 1000.0;
    for (int i = imin; i <= imax; ++i) {
        const double nb = (i / 1000.0 - b0) / (b1 - b0);
        std_curve[i] = sqrt(nb * (s_hi * s_hi - s_lo * s_lo) + s_lo * s_lo);
        diff_curve[i] = sqrt(nb * (d_hi * d_hi - d_lo * d_lo) + d_lo * d_lo);
    }
    return 0;
}
