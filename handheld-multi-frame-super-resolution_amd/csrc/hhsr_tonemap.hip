// Tone mapping on the device (reference raw2rgb.py:153-170): exposure fusion of n uint8 exposures of the finished image —
// OpenCV 4.x MergeMertens with createMergeMertens() defaults, restated operation by operation in include/hhsr.h and
// tests/mertens_ref.py — and the smoothstep curve.  Three kinds of kernel: the weight maps (a decision stage: float32,
// exact association, no contraction), one decimation per pyramid level (colour + weight of every exposure), and one
// collapse per level from coarse to fine that forms the Laplacian in registers and never stores it.
#include "hhsr_common.h"
#include <math.h>

#define TM_MAX_LEVELS 32
#define TM_TX 32        // output tile of the down / up kernels: 32 x 8 pixels, one per thread
#define TM_TY 8

// ---- host: pyramid geometry and workspace layout ----------------------------------------------------------------------
// workspace = wn level 0 [n][H][W] | per level l = 1..L: G_l [n][4][h][w] (R, G, B, weight), R_l [3][h][w]; float32,
// every block 256-byte aligned
struct TmPlan {
    int L;
    int h[TM_MAX_LEVELS], w[TM_MAX_LEVELS];
    size_t g_off[TM_MAX_LEVELS], r_off[TM_MAX_LEVELS];  // in floats
    size_t bytes;
};

static inline size_t tm_align(size_t floats) { return (floats + 63) & ~(size_t)63; }

static void tm_plan(int H, int W, int n, TmPlan& p) {
    // OpenCV: int(logf(float(min(rows, cols))) / logf(2.f)) = floor(log2(min)), except that in float32 the quotient at a
    // power of two is within a rounding of an integer and follows the platform's logf (12 at 8192 with a correctly
    // rounded one).  The contract is the table: L = k for 2^k <= min < 2^(k + 1).
    p.L = 0;
    for (int m = H < W ? H : W; m > 1; m >>= 1) ++p.L;
    p.h[0] = H;
    p.w[0] = W;
    size_t off = tm_align((size_t)n * H * W);
    p.g_off[0] = p.r_off[0] = 0;
    for (int l = 1; l <= p.L; ++l) {
        p.h[l] = (p.h[l - 1] + 1) / 2;
        p.w[l] = (p.w[l - 1] + 1) / 2;
        const size_t hw = (size_t)p.h[l] * p.w[l];
        p.g_off[l] = off;
        off += tm_align((size_t)n * 4 * hw);
        p.r_off[l] = off;
        off += tm_align(3 * hw);
    }
    p.bytes = off * sizeof(float);
}

// ---- device helpers ---------------------------------------------------------------------------------------------------
// BORDER_REFLECT_101 (d c b | a b c d | c b a), repeated until the index is in range; 0 on an axis of length 1
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// pyrUp's source index: s[-1] := s[1] (s[0] on an axis of length 1), s[n] := s[n - 1]
__device__ __forceinline__ int up_index(int i, int n) { return i < 0 ? (n > 1 ? 1 : 0) : (i >= n ? n - 1 : i); }

__device__ __forceinline__ float u8f(uint8_t e) { return (float)e * (float)(1.0 / 255.0); }

// ---- weight maps ----------------------------------------------------------------------------------------------------------
// 64 x 4 pixels per workgroup; the grey image of every exposure goes to LDS with a one-pixel halo
__global__ void __launch_bounds__(256) k_tm_weights(const uint8_t* __restrict__ expo, int n, int H, int W,
                                                     float* __restrict__ wn, float* __restrict__ wn_copy) {
    __shared__ float grey[HHSR_MAX_EXPOSURES][6][66];
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 4;
    const size_t plane = (size_t)H * W;
    for (int idx = threadIdx.x; idx < 6 * 66; idx += 256) {
        const int ly = idx / 66, lx = idx - ly * 66;
        const size_t o = ((size_t)reflect101(y0 - 1 + ly, H) * W + reflect101(x0 - 1 + lx, W)) * 3;
#pragma unroll
        for (int i = 0; i < HHSR_MAX_EXPOSURES; ++i)
            if (i < n) {
                const uint8_t* p = expo + (size_t)i * plane * 3 + o;
                grey[i][ly][lx] = (u8f(p[0]) * 0.299f + u8f(p[1]) * 0.587f) + u8f(p[2]) * 0.114f;
            }
    }
    __syncthreads();
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6, x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const size_t o = (size_t)y * W + x;
    float w[HHSR_MAX_EXPOSURES];
    float ws = 0.f;
#pragma unroll
    for (int i = 0; i < HHSR_MAX_EXPOSURES; ++i)
        if (i < n) {
            const float (*g)[66] = grey[i];
            const float contrast = fabsf((((g[ly][lx + 1] + g[ly + 1][lx]) + g[ly + 1][lx + 1] * -4.f) + g[ly + 1][lx + 2]) + g[ly + 2][lx + 1]);
            const uint8_t* p = expo + ((size_t)i * plane + o) * 3;
            const float I0 = u8f(p[0]), I1 = u8f(p[1]), I2 = u8f(p[2]);
            const float mean = ((I0 + I1) + I2) * (float)(1.0 / 3.0);
            const float d0 = I0 - mean, d1 = I1 - mean, d2 = I2 - mean;
            const float saturation = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);  // correctly rounded (hipcc's default)
            w[i] = contrast * saturation + 1e-12f;
            ws = i == 0 ? w[i] : ws + w[i];
        }
#pragma unroll
    for (int i = 0; i < HHSR_MAX_EXPOSURES; ++i)
        if (i < n) {
            const float v = w[i] / ws;  // correctly rounded (hipcc's default)
            wn[(size_t)i * plane + o] = v;
            if (wn_copy) wn_copy[(size_t)i * plane + o] = v;
        }
}

// ---- pyrDown of the 3 colours and the weight of one exposure ------------------------------------------------------
// A workgroup makes 32 x 8 samples of level l + 1 from a 67 x 19 window of level l: window -> LDS, 5 taps along x ->
// LDS, 5 taps along y, x 1/256 (OpenCV's order).  L0: level 0 is the uint8 exposure and the wn plane.
#define TM_DW (2 * TM_TX + 3)
#define TM_DH (2 * TM_TY + 3)
template <bool L0>
__global__ void __launch_bounds__(256) k_tm_down(const uint8_t* __restrict__ expo, const float* __restrict__ wn,
                                                  const float* __restrict__ src, int h, int w, float* __restrict__ dst,
                                                  int oh, int ow) {
    __shared__ float win[4][TM_DH][TM_DW];
    __shared__ float hz[4][TM_DH][TM_TX + 1];
    const int e = blockIdx.z, ox0 = blockIdx.x * TM_TX, oy0 = blockIdx.y * TM_TY;
    const size_t plane = (size_t)h * w;
    for (int idx = threadIdx.x; idx < TM_DH * TM_DW; idx += 256) {
        const int ly = idx / TM_DW, lx = idx - ly * TM_DW;
        const size_t o = (size_t)reflect101(2 * oy0 - 2 + ly, h) * w + reflect101(2 * ox0 - 2 + lx, w);
        if (L0) {
            const uint8_t* p = expo + ((size_t)e * plane + o) * 3;
            win[0][ly][lx] = u8f(p[0]);
            win[1][ly][lx] = u8f(p[1]);
            win[2][ly][lx] = u8f(p[2]);
            win[3][ly][lx] = wn[(size_t)e * plane + o];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) win[c][ly][lx] = src[((size_t)e * 4 + c) * plane + o];
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 4 * TM_DH * TM_TX; idx += 256) {
        const int ox = idx & (TM_TX - 1), ly = (idx / TM_TX) % TM_DH, c = idx / (TM_TX * TM_DH);
        const float* s = &win[c][ly][2 * ox];
        hz[c][ly][ox] = ((s[2] * 6.f + (s[1] + s[3]) * 4.f) + s[0]) + s[4];
    }
    __syncthreads();
    const int lx = threadIdx.x & (TM_TX - 1), ly = threadIdx.x / TM_TX, ox = ox0 + lx, oy = oy0 + ly;
    if (ox >= ow || oy >= oh) return;
    const size_t oplane = (size_t)oh * ow, oo = (size_t)oy * ow + ox;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float r0 = hz[c][2 * ly][lx], r1 = hz[c][2 * ly + 1][lx], r2 = hz[c][2 * ly + 2][lx], r3 = hz[c][2 * ly + 3][lx],
                    r4 = hz[c][2 * ly + 4][lx];
        dst[((size_t)e * 4 + c) * oplane + oo] = (((r2 * 6.f + (r1 + r3) * 4.f) + r0) + r4) * (1.f / 256.f);
    }
}

// ---- collapse: out_l = sum_i (G_l^i - pyrUp(G_{l+1}^i)) W_l^i + pyrUp(out_{l+1}) ------------------------------------
// A workgroup makes 32 x 8 pixels of level l.  The 18 x 6 window of level l + 1 they depend on — 3 colours of every
// exposure and the 3 channels of out_{l+1}, border rule applied — goes to LDS, is expanded along x into LDS, and every
// thread expands along y for its own pixel.  TOP: the coarsest level, out_L = sum_i G_L^i W_L^i.  L0: level 0 reads the
// uint8 exposures and the wn plane and stores interleaved [H][W][3], with the smoothstep curve when asked.
#define TM_UW (TM_TX / 2 + 2)
#define TM_UH (TM_TY / 2 + 2)
#define TM_UP (3 * HHSR_MAX_EXPOSURES + 3)
template <bool L0, bool TOP>
__global__ void __launch_bounds__(256) k_tm_up(const uint8_t* __restrict__ expo, const float* __restrict__ wn,
                                                const float* __restrict__ g, int n, int h, int w,
                                                const float* __restrict__ gc, const float* __restrict__ rc, int ch, int cw,
                                                float* __restrict__ out, int smoothstep) {
    __shared__ float cs[TOP ? 1 : TM_UP][TM_UH][TM_UW];
    __shared__ float hx[TOP ? 1 : TM_UP][TM_UH][TM_TX + 1];
    const int x0 = blockIdx.x * TM_TX, y0 = blockIdx.y * TM_TY;
    const int lx = threadIdx.x & (TM_TX - 1), ly = threadIdx.x / TM_TX, x = x0 + lx, y = y0 + ly;
    const int np = 3 * n + 3;  // planes of level l + 1: [i][c] of the exposures, then out_{l+1}
    if (!TOP) {
        const size_t cplane = (size_t)ch * cw;
        for (int idx = threadIdx.x; idx < np * TM_UH * TM_UW; idx += 256) {
            const int sx = idx % TM_UW, sy = (idx / TM_UW) % TM_UH, p = idx / (TM_UW * TM_UH);
            const size_t o = (size_t)up_index(y0 / 2 - 1 + sy, ch) * cw + up_index(x0 / 2 - 1 + sx, cw);
            cs[p][sy][sx] = p < 3 * n ? gc[((size_t)(p / 3) * 4 + p % 3) * cplane + o] : rc[(size_t)(p - 3 * n) * cplane + o];
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < np * TM_UH * TM_TX; idx += 256) {
            const int xx = idx & (TM_TX - 1), sy = (idx / TM_TX) % TM_UH, p = idx / (TM_TX * TM_UH);
            const float* s = &cs[p][sy][(xx >> 1) + 1];  // s[0] = source sample xx / 2 of this tile
            hx[p][sy][xx] = (xx & 1) ? (s[0] + s[1]) * 4.f : (s[-1] + s[0] * 6.f) + s[1];
        }
        __syncthreads();
    }
    if (x >= w || y >= h) return;
    const size_t plane = (size_t)h * w, o = (size_t)y * w + x;
    const int j = (ly >> 1) + 1;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < HHSR_MAX_EXPOSURES; ++i)
        if (i < n) {
            float v[3], wt;
            if (L0) {
                const uint8_t* p = expo + ((size_t)i * plane + o) * 3;
                v[0] = u8f(p[0]);
                v[1] = u8f(p[1]);
                v[2] = u8f(p[2]);
                wt = wn[(size_t)i * plane + o];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = g[((size_t)i * 4 + c) * plane + o];
                wt = g[((size_t)i * 4 + 3) * plane + o];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float lap = v[c];
                if (!TOP) {
                    const int p = 3 * i + c;
                    const float up = (ly & 1) ? (hx[p][j][lx] + hx[p][j + 1][lx]) * 4.f
                                              : (hx[p][j - 1][lx] + hx[p][j][lx] * 6.f) + hx[p][j + 1][lx];
                    lap = v[c] - up * (1.f / 64.f);
                }
                const float t = lap * wt;
                acc[c] = i == 0 ? t : acc[c] + t;
            }
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float r = acc[c];
        if (!TOP) {
            const int p = 3 * n + c;
            const float up = (ly & 1) ? (hx[p][j][lx] + hx[p][j + 1][lx]) * 4.f
                                      : (hx[p][j - 1][lx] + hx[p][j][lx] * 6.f) + hx[p][j + 1][lx];
            r = r + up * (1.f / 64.f);
        }
        if (L0) {
            if (smoothstep) r = 3.f * (r * r) - 2.f * (r * r * r);  // raw2rgb.py:169
            out[o * 3 + c] = r;
        } else {
            out[(size_t)c * plane + o] = r;
        }
    }
}

// ---- C ABI ----------------------------------------------------------------------------------------------------------------
static bool tm_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

extern "C" int hhsr_tonemap_workspace(int H, int W, int n, size_t* bytes, int* levels) {
    HHSR_ARG(H > 0 && W > 0 && n >= 1 && n <= HHSR_MAX_EXPOSURES && bytes && levels);
    HHSR_ARG((size_t)H * W * 3 < ((size_t)1 << 31));
    TmPlan p;
    tm_plan(H, W, n, p);
    *bytes = p.bytes;
    *levels = p.L;
    return 0;
}

extern "C" int hhsr_mertens(const uint8_t* exposures, int n, int H, int W, void* workspace, size_t workspace_bytes,
                            float* weights_out, float* out, int smoothstep, void* stream) {
    HHSR_ARG(exposures && workspace && out);
    HHSR_ARG(n >= 1 && n <= HHSR_MAX_EXPOSURES && H > 0 && W > 0);
    HHSR_ARG((size_t)H * W * 3 < ((size_t)1 << 31));
    HHSR_ARG(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)weights_out & 3) == 0);
    TmPlan p;
    tm_plan(H, W, n, p);
    HHSR_ARG(workspace_bytes >= p.bytes);
    const size_t hw = (size_t)H * W, eb = (size_t)n * hw * 3, ob = hw * 3 * sizeof(float), wb = (size_t)n * hw * sizeof(float);
    HHSR_ARG(!tm_overlap(exposures, eb, workspace, p.bytes) && !tm_overlap(exposures, eb, out, ob) &&
             !tm_overlap(workspace, p.bytes, out, ob));
    HHSR_ARG(!weights_out || (!tm_overlap(weights_out, wb, exposures, eb) && !tm_overlap(weights_out, wb, workspace, p.bytes) &&
                              !tm_overlap(weights_out, wb, out, ob)));
    hipStream_t s = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* wn = ws;
    const dim3 block(256);
    hipLaunchKernelGGL(k_tm_weights, dim3(hhsr_cdiv(W, 64), hhsr_cdiv(H, 4)), block, 0, s, exposures, n, H, W, wn, weights_out);
    for (int l = 0; l < p.L; ++l) {
        const dim3 grid(hhsr_cdiv(p.w[l + 1], TM_TX), hhsr_cdiv(p.h[l + 1], TM_TY), n);
        if (l == 0)
            hipLaunchKernelGGL(k_tm_down<true>, grid, block, 0, s, exposures, (const float*)wn, (const float*)nullptr, H, W,
                               ws + p.g_off[1], p.h[1], p.w[1]);
        else
            hipLaunchKernelGGL(k_tm_down<false>, grid, block, 0, s, (const uint8_t*)nullptr, (const float*)nullptr,
                               (const float*)(ws + p.g_off[l]), p.h[l], p.w[l], ws + p.g_off[l + 1], p.h[l + 1], p.w[l + 1]);
    }
    for (int l = p.L; l >= 0; --l) {
        const dim3 grid(hhsr_cdiv(p.w[l], TM_TX), hhsr_cdiv(p.h[l], TM_TY));
        const bool top = l == p.L;
        const float* g = l ? ws + p.g_off[l] : nullptr;
        const float* gc = top ? nullptr : ws + p.g_off[l + 1];
        const float* rc = top ? nullptr : ws + p.r_off[l + 1];
        const int ch = top ? 0 : p.h[l + 1], cw = top ? 0 : p.w[l + 1];
        float* o = l ? ws + p.r_off[l] : out;
        if (l == 0 && top)
            hipLaunchKernelGGL((k_tm_up<true, true>), grid, block, 0, s, exposures, (const float*)wn, g, n, H, W, gc, rc, ch, cw, o, smoothstep);
        else if (l == 0)
            hipLaunchKernelGGL((k_tm_up<true, false>), grid, block, 0, s, exposures, (const float*)wn, g, n, H, W, gc, rc, ch, cw, o, smoothstep);
        else if (top)
            hipLaunchKernelGGL((k_tm_up<false, true>), grid, block, 0, s, (const uint8_t*)nullptr, (const float*)nullptr, g, n, p.h[l], p.w[l], gc, rc, ch, cw, o, 0);
        else
            hipLaunchKernelGGL((k_tm_up<false, false>), grid, block, 0, s, (const uint8_t*)nullptr, (const float*)nullptr, g, n, p.h[l], p.w[l], gc, rc, ch, cw, o, 0);
    }
    HHSR_LAUNCHED();
}
