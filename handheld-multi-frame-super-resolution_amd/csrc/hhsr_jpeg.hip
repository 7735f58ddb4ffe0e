// JPEG output (include/hhsr.h "JPEG output"): the finished float32 image -> the entropy-coded scan of a baseline JFIF file,
// both stages on the device, so that what crosses the host link is the file and not its samples.  The reference writes its
// JPEG on the host (run_handheld.py: imsave = cv2.imwrite) after the float32 image crossed the link.
//
// k_jpeg_dct   12 B in, 6 B out per RGB pixel and some 50 flops: bandwidth-shaped.  A workgroup takes 8 image rows x 32 MCUs
//              (256 columns): thread t loads column t of the 8 rows — a pixel is 4 or 12 consecutive bytes and the lanes of
//              a load are consecutive pixels, so every load instruction of a wave reads 256 / 768 consecutive bytes of one
//              row without asking anything of the image's alignment; the clamped index IS the edge replication —
//              quantises and colour-transforms it and leaves the three planes in LDS.  One thread per ROW pass of a block,
//              then one thread per COLUMN pass (768 of each for RGB: three per thread), in place in LDS: a lane group per
//              block would need cross-lane butterflies for the same 8-point transforms, and a whole block per thread holds
//              64 live values per lane for a kernel whose limit is bandwidth.  The column pass reads LDS at stride 1 across
//              the wave (conflict-free); the row pass reads 8 consecutive floats per lane as two b128 (lanes 32 bytes apart:
//              2-way).  Quantised values go to LDS in zig-zag order and leave as 16-byte stores: a workgroup's 32 MCUs are
//              one contiguous piece of the coefficient array.
// k_jpeg_scan  one wave per restart interval, a lane per block, 64 blocks at a time.  A lane walks its block twice: once
//              for the length of its bit string, then — after a wave prefix sum over the lengths has placed it — to OR the
//              string into the wave's LDS bit buffer (bitwise OR commutes: the buffer's content does not depend on the
//              order of the lanes).  The wave then reads the buffer back a byte per lane and counts (SIZE pass) or stores
//              (WRITE pass) the bytes, 0xFF followed by 0x00, at positions a ballot gives.  Between the two passes one
//              exclusive scan over the intervals' byte counts (three small kernels) gives every interval its offset, so
//              the write pass stores every byte at its final place and compares every position with the capacity.
//              No global atomics anywhere: the bytes are a function of the coefficients alone.
// Extended ("JPEG output, extended"): k_jpeg_dct420 (4:2:0: 16 rows x 256 columns per workgroup, chroma averaged over 2 x 2
// pixels), k_jpeg_scan<WRITE, true> (any MCU layout, code words from a kernel argument) and k_jpeg_histogram (the scan's
// symbol counts for hhsr_jpeg_huffman).  The tables, K.2 and the header writer are in hhsr_jpeg_tables.h, free of HIP.
#include "hhsr_common.h"
#include "hhsr_jpeg_tables.h"
#include "hhsr_scan.h"  // (the offsets scan below is declared there: hhsr_png.hip launches it too)

// ---- tables, geometry, header writer: hhsr_jpeg_tables.h (no HIP in it) -------------------------------------------------
using jpeg::HuffCodes;
using jpeg::HuffSpec;
using jpeg::HUFF_WORDS;
using jpeg::SCAN_GROUP;

__device__ const HuffCodes d_huff = jpeg::huff_codes(jpeg::STANDARD_SPECS);
__device__ const uint8_t d_zigzag[64] = JPEG_ZIGZAG;
__device__ const uint8_t d_base_q[2][64] = {JPEG_K1_LUMA, JPEG_K2_CHROMA};

#define JPEG_ARG_DIMS() \
    HHSR_ARG(H > 0 && W > 0 && H <= jpeg::MAX_DIM && W <= jpeg::MAX_DIM)

static inline bool jpeg_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}

#define JPEG_ARG_SUB() \
    HHSR_ARG((subsampling == 0 || subsampling == 1) && (subsampling == 0 || out_channels == 3))

// ---- header, workspace, table construction (host only) ------------------------------------------------------------------------
extern "C" int hhsr_jpeg_header_ex(int H, int W, int out_channels, int quality, int restart_mcus, int subsampling,
                                   const uint8_t* spec, uint8_t* out, size_t out_capacity, size_t* length) {
    HHSR_ARG(out != nullptr && length != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(quality >= 1 && quality <= 100);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    JPEG_ARG_SUB();
    HuffSpec store[4];
    const HuffSpec* specs[4];
    const bool spec_is_valid = jpeg::specs_from_abi(spec, out_channels == 1 ? 2 : 4, store, specs);
    HHSR_ARG(spec_is_valid);
    const int rc = jpeg::write_header(H, W, out_channels, quality, restart_mcus, subsampling, specs, out, out_capacity, length);
    HHSR_ARG(rc != 1 /* out_capacity >= *length */);
    if (rc != 0) {
        hhsr_set_error("hhsr_jpeg_header: internal length mismatch");
        return -2;
    }
    return 0;
}

extern "C" int hhsr_jpeg_header(int H, int W, int out_channels, int quality, int restart_mcus, uint8_t* out,
                                size_t out_capacity, size_t* length) {
    return hhsr_jpeg_header_ex(H, W, out_channels, quality, restart_mcus, 0, nullptr, out, out_capacity, length);
}

extern "C" int hhsr_jpeg_workspace_ex(int H, int W, int out_channels, int restart_mcus, int subsampling, size_t* coef_bytes,
                                      size_t* scratch_bytes, size_t* max_scan_bytes) {
    HHSR_ARG(coef_bytes != nullptr && scratch_bytes != nullptr && max_scan_bytes != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    JPEG_ARG_SUB();
    const jpeg::Geom g = jpeg::geom(H, W, out_channels, restart_mcus, subsampling);
    *coef_bytes = g.coef_bytes;
    *scratch_bytes = g.scratch_bytes > g.hist_bytes ? g.scratch_bytes : g.hist_bytes;  // entropy coder | histogram
    *max_scan_bytes = g.max_scan;
    return 0;
}

extern "C" int hhsr_jpeg_workspace(int H, int W, int out_channels, int restart_mcus, size_t* coef_bytes,
                                   size_t* scratch_bytes, size_t* max_scan_bytes) {
    HHSR_ARG(coef_bytes != nullptr && scratch_bytes != nullptr && max_scan_bytes != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    const jpeg::Geom g = jpeg::geom(H, W, out_channels, restart_mcus);
    *coef_bytes = g.coef_bytes;
    *scratch_bytes = g.scratch_bytes;
    *max_scan_bytes = g.max_scan;
    return 0;
}

extern "C" int hhsr_jpeg_huffman(const uint64_t* counts, int n_tables, uint8_t* spec) {
    HHSR_ARG(counts != nullptr && spec != nullptr);
    HHSR_ARG(n_tables == 2 || n_tables == 4);
    HHSR_ARG(((uintptr_t)counts & 7) == 0);
    HHSR_ARG(jpeg_disjoint(counts, (size_t)n_tables * 256 * sizeof(uint64_t), spec, (size_t)n_tables * jpeg::SPEC_BYTES));
    uint8_t built[4][jpeg::SPEC_BYTES];
    for (int t = 0; t < n_tables; ++t) {
        const bool counts_are_usable = jpeg::huffman_build(counts + (size_t)t * 256, built[t]);
        HHSR_ARG(counts_are_usable /* a table's counts: not all zero, their sum below 2^64 */);
    }
    for (int t = 0; t < n_tables; ++t)
        for (int k = 0; k < jpeg::SPEC_BYTES; ++k) spec[(size_t)t * jpeg::SPEC_BYTES + k] = built[t][k];
    return 0;
}

// ---- transform ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float jpeg_sample(float x) {  // the 8-bit rule of hhsr_encode_image: an integer in [0, 255]
    x = x == x ? x : 0.f;
    x = fminf(fmaxf(x, 0.f), 1.f);
    return rintf(x * 255.f);
}

// 8-point DCT-II of A.3.3 (X_u = C(u) / 2 sum_n x_n cos((2 n + 1) u pi / 16)), even / odd halves: 22 multiplies
__device__ __forceinline__ void dct8(float* x) {
    constexpr float c1 = 0.98078528040323044913f, c2 = 0.92387953251128675613f, c3 = 0.83146961230254523708f,
                    c4 = 0.70710678118654752440f, c5 = 0.55557023301960222474f, c6 = 0.38268343236508977173f,
                    c7 = 0.19509032201612826785f;
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const float e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
    x[0] = (0.5f * c4) * (e0 + e1);
    x[4] = (0.5f * c4) * (e0 - e1);
    x[2] = 0.5f * (c2 * e2 + c6 * e3);
    x[6] = 0.5f * (c6 * e2 - c2 * e3);
    x[1] = 0.5f * (c1 * d0 + c3 * d1 + c5 * d2 + c7 * d3);
    x[3] = 0.5f * (c3 * d0 - c7 * d1 - c1 * d2 - c5 * d3);
    x[5] = 0.5f * (c5 * d0 - c1 * d1 + c7 * d2 + c3 * d3);
    x[7] = 0.5f * (c7 * d0 - c5 * d1 + c3 * d2 - c1 * d3);
}

// A block's row pass, in place: 8 consecutive floats as two b128
__device__ __forceinline__ void dct_row_pass(float* row) {
    float4 a = reinterpret_cast<float4*>(row)[0], b = reinterpret_cast<float4*>(row)[1];
    float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    dct8(x);
    reinterpret_cast<float4*>(row)[0] = make_float4(x[0], x[1], x[2], x[3]);
    reinterpret_cast<float4*>(row)[1] = make_float4(x[4], x[5], x[6], x[7]);
}

// Column v of a block (8 floats `pitch` apart), then the division by q (row-major) into o at the zig-zag positions
__device__ __forceinline__ void dct_col_pass(const float* col, int pitch, int v, const float* q, const uint8_t* zpos,
                                             int16_t* o) {
    float x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = col[u * pitch];
    dct8(x);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int k = u * 8 + v;
        const float lo = k == 0 ? -1024.f : -1023.f;
        o[zpos[k]] = (int16_t)fminf(fmaxf(rintf(x[u] / q[k]), lo), 1023.f);
    }
}

constexpr int DCT_MCUS = 32;                   // MCUs (= blocks of a component) per workgroup: 256 columns
constexpr int DCT_PITCH = DCT_MCUS * 8 + 4;    // floats per LDS row: 16-byte aligned rows

// NC components from an image of STEP floats per pixel (STEP 3, NC 1: channel 0 alone)
template <int NC, int STEP>
__global__ void __launch_bounds__(256) k_jpeg_dct(const float* __restrict__ image, int H, int W, int mcux, int scale,
                                                   int16_t* __restrict__ coef) {
    __shared__ __attribute__((aligned(16))) float P[NC][8][DCT_PITCH];
    __shared__ __attribute__((aligned(16))) int16_t O[DCT_MCUS * NC * 64];
    __shared__ float Q[NC == 1 ? 1 : 2][64];  // divisors, row-major
    __shared__ uint8_t zpos[64];              // row-major index -> zig-zag position
    const int t = threadIdx.x, bx0 = blockIdx.x * DCT_MCUS, by = blockIdx.y;
    if (t < 64) zpos[d_zigzag[t]] = (uint8_t)t;
    if (t < 64 * (NC == 1 ? 1 : 2)) Q[t >> 6][t & 63] = (float)jpeg::q_entry(d_base_q[t >> 6][t & 63], scale);
    {
        const int xs = min(bx0 * 8 + t, W - 1);  // replication of the last column
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int ys = min(by * 8 + r, H - 1);  // ... and of the last row
            const float* __restrict__ p = image + ((size_t)ys * W + xs) * STEP;
            if constexpr (NC == 1) {
                P[0][r][t] = jpeg_sample(p[0]) - 128.f;
            } else {
                const float R = jpeg_sample(p[0]), G = jpeg_sample(p[1]), B = jpeg_sample(p[2]);
                P[0][r][t] = 0.299f * R + 0.587f * G + 0.114f * B - 128.f;
                P[1][r][t] = -0.168736f * R - 0.331264f * G + 0.5f * B;
                P[2][r][t] = 0.5f * R - 0.418688f * G - 0.081312f * B;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = t; i < NC * 256; i += 256)  // row passes: (component, row, block)
        dct_row_pass(&P[i >> 8][(i >> 5) & 7][(i & 31) * 8]);
    __syncthreads();
#pragma unroll
    for (int i = t; i < NC * 256; i += 256) {  // column passes: (component, block, column), then the division
        const int c = i >> 8, col = i & 255, b = col >> 3;
        dct_col_pass(&P[c][0][col], DCT_PITCH, col & 7, Q[c ? 1 : 0], zpos, &O[(b * NC + c) * 64]);
    }
    __syncthreads();
    const int nvalid = min(DCT_MCUS, mcux - bx0);  // MCUs of this workgroup that exist
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(coef + ((size_t)by * mcux + bx0) * (NC * 64));
    for (int i = t; i < nvalid * NC * 8; i += 256) dst[i] = reinterpret_cast<const uint4*>(O)[i];
}

// 4:2:0: a workgroup takes 16 image rows x 256 columns = 16 MCUs.  Thread t loads column t of the 16 rows; Y goes to LDS
// as 2 x 32 blocks with the arithmetic of k_jpeg_dct; Cb and Cr stay unrounded float32, and a chroma sample is
// 0.25 ((c00 + c01) + (c10 + c11)): the horizontal sums come from the neighbouring lane (c + its neighbour is the same sum in
// both lanes of a pair), the even lane adds the two rows' sums.  96 blocks, 768 row and 768 column passes: three of each per
// thread, as RGB 4:4:4.  O holds the 16 MCUs in coding order: Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr.
constexpr int DCT420_MCUS = 16;
constexpr int DCT420_CPITCH = DCT420_MCUS * 8 + 4;

__global__ void __launch_bounds__(256) k_jpeg_dct420(const float* __restrict__ image, int H, int W, int mcux, int scale,
                                                      int16_t* __restrict__ coef) {
    __shared__ __attribute__((aligned(16))) float Y[16][DCT_PITCH];
    __shared__ __attribute__((aligned(16))) float C[2][8][DCT420_CPITCH];
    __shared__ __attribute__((aligned(16))) int16_t O[DCT420_MCUS * 6 * 64];
    __shared__ float Q[2][64];
    __shared__ uint8_t zpos[64];
    const int t = threadIdx.x, bx0 = blockIdx.x * DCT420_MCUS, by = blockIdx.y;
    if (t < 64) zpos[d_zigzag[t]] = (uint8_t)t;
    if (t < 128) Q[t >> 6][t & 63] = (float)jpeg::q_entry(d_base_q[t >> 6][t & 63], scale);
    {
        const int xs = min(bx0 * 16 + t, W - 1);  // replication of the last column
#pragma unroll
        for (int r2 = 0; r2 < 8; ++r2) {
            float hb[2], hr[2];  // cb, cr: this column + its neighbour, rows 2 r2 and 2 r2 + 1
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int r = 2 * r2 + k;
                const int ys = min(by * 16 + r, H - 1);  // ... and of the last row
                const float* __restrict__ p = image + ((size_t)ys * W + xs) * 3;
                const float R = jpeg_sample(p[0]), G = jpeg_sample(p[1]), B = jpeg_sample(p[2]);
                Y[r][t] = 0.299f * R + 0.587f * G + 0.114f * B - 128.f;
                const float cb = -0.168736f * R - 0.331264f * G + 0.5f * B;
                const float cr = 0.5f * R - 0.418688f * G - 0.081312f * B;
                const float nb = __shfl_xor(cb, 1, 64), nr = __shfl_xor(cr, 1, 64);
                hb[k] = cb + nb;  // (the pair's sum in both of its lanes: float addition commutes)
                hr[k] = cr + nr;
            }
            if ((t & 1) == 0) {
                C[0][r2][t >> 1] = 0.25f * (hb[0] + hb[1]);
                C[1][r2][t >> 1] = 0.25f * (hr[0] + hr[1]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = t; i < 768; i += 256) {  // row passes: Y (row, block) x 512, then (component, row, block) x 256
        if (i < 512) dct_row_pass(&Y[i >> 5][(i & 31) * 8]);
        else dct_row_pass(&C[(i >> 7) & 1][(i >> 4) & 7][(i & 15) * 8]);
    }
    __syncthreads();
#pragma unroll
    for (int i = t; i < 768; i += 256) {  // column passes
        if (i < 512) {                    // Y: (block row, column); block b of the row is Y(row, b & 1) of MCU b >> 1
            const int br = i >> 8, col = i & 255, b = col >> 3;
            dct_col_pass(&Y[br * 8][col], DCT_PITCH, col & 7, Q[0], zpos, &O[((b >> 1) * 6 + br * 2 + (b & 1)) * 64]);
        } else {                          // Cb, Cr: (component, column); block b is MCU b's
            const int c = (i >> 7) & 1, col = i & 127;
            dct_col_pass(&C[c][0][col], DCT420_CPITCH, col & 7, Q[1], zpos, &O[((col >> 3) * 6 + 4 + c) * 64]);
        }
    }
    __syncthreads();
    const int nvalid = min(DCT420_MCUS, mcux - bx0);  // MCUs of this workgroup that exist
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(coef + ((size_t)by * mcux + bx0) * (6 * 64));
    for (int i = t; i < nvalid * 6 * 8; i += 256) dst[i] = reinterpret_cast<const uint4*>(O)[i];
}

extern "C" int hhsr_jpeg_dct_ex(const float* image, int H, int W, int channels, int out_channels, int quality,
                                int subsampling, int16_t* coef, size_t coef_bytes, void* stream) {
    HHSR_ARG(image != nullptr && coef != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(channels == 1 || channels == 3);
    HHSR_ARG(out_channels == channels || out_channels == 1);
    HHSR_ARG(quality >= 1 && quality <= 100);
    JPEG_ARG_SUB();
    HHSR_ARG(((uintptr_t)image & 3) == 0 && ((uintptr_t)coef & 15) == 0);
    const jpeg::Geom g = jpeg::geom(H, W, out_channels, 1, subsampling);
    HHSR_ARG(coef_bytes >= g.coef_bytes);
    HHSR_ARG(jpeg_disjoint(image, (size_t)H * W * channels * sizeof(float), coef, g.coef_bytes));
    const dim3 grid((unsigned)hhsr_cdiv(g.mcux, subsampling ? DCT420_MCUS : DCT_MCUS), (unsigned)g.mcuy), block(256);
    const int scale = jpeg::q_scale(quality);
#define HHSR_JPEG_DCT(KERNEL) \
    hipLaunchKernelGGL(KERNEL, grid, block, 0, (hipStream_t)stream, image, H, W, g.mcux, scale, coef)
    if (subsampling) HHSR_JPEG_DCT(k_jpeg_dct420);
    else if (out_channels == 3) HHSR_JPEG_DCT((k_jpeg_dct<3, 3>));
    else if (channels == 3) HHSR_JPEG_DCT((k_jpeg_dct<1, 3>));
    else HHSR_JPEG_DCT((k_jpeg_dct<1, 1>));
#undef HHSR_JPEG_DCT
    HHSR_LAUNCHED();
}

extern "C" int hhsr_jpeg_dct(const float* image, int H, int W, int channels, int out_channels, int quality, int16_t* coef,
                             size_t coef_bytes, void* stream) {
    return hhsr_jpeg_dct_ex(image, H, W, channels, out_channels, quality, 0, coef, coef_bytes, stream);
}

// ---- entropy coding -----------------------------------------------------------------------------------------------------------
// Bits of a wave's 64 blocks: at most 7 carried bits + 64 x (22 DC + 63 x 26 AC) = 106247 bits = 3321 words.
constexpr int SCAN_WORDS = 3328;

__device__ __forceinline__ int jpeg_clamp_coef(int v, bool dc) { return max(dc ? -1024 : -1023, min(v, 1023)); }

// A block's symbols in coding order through sym(is_ac, symbol, value, size): the DC difference (symbol = its category), then
// per non-zero AC value ZRL (0xF0) for every 16 zeros before it and run << 4 | size, and EOB (0x00) if the block ends in zeros.
template <typename Sym>
__device__ __forceinline__ void jpeg_walk_block(const int16_t* __restrict__ blk, int pred, Sym sym) {
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 w = reinterpret_cast<const uint4*>(blk)[g];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int raw = (int)(int16_t)(ws[j >> 1] >> ((j & 1) * 16));
            if (g == 0 && j == 0) {
                const int d = jpeg_clamp_coef(raw, true) - pred;       // |d| <= 2047: category <= 11 < 16
                const int cat = 32 - __clz(abs(d));
                sym(false, cat, d, cat);
            } else {
                const int v = jpeg_clamp_coef(raw, false);             // |v| <= 1023: size <= 10
                if (v == 0) {
                    ++run;
                } else {
                    while (run >= 16) {
                        sym(true, 0xF0, 0, 0);
                        run -= 16;
                    }
                    const int cat = 32 - __clz(abs(v));
                    sym(true, (run << 4) | cat, v, cat);                // run <= 15, cat <= 10: < 256
                    run = 0;
                }
            }
        }
    }
    if (run) sym(true, 0, 0, 0);
}

// A block's bit string, symbol by symbol, through put(bits, count): count <= 26, bits < 2^count.  Returns whether the
// block needed a symbol the tables do not have (entry 0: nothing but the magnitude bits is put for it).
template <typename Put>
__device__ __forceinline__ bool jpeg_code_block(const int16_t* __restrict__ blk, int pred, const uint32_t* __restrict__ dc,
                                                const uint32_t* __restrict__ ac, Put put) {
    bool missing = false;
    jpeg_walk_block(blk, pred, [&](bool is_ac, int s, int v, int cat) {
        const uint32_t e = (is_ac ? ac : dc)[s];
        missing |= e == 0;
        put((e & 0xffffu) << cat | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << cat) - 1)), (int)(e >> 16) + cat);
    });
    return missing;
}

// One wave per restart interval.  WRITE false: sizes[interval] = its bytes (stuffing, padding and RSTm included).
// WRITE true: the bytes to scan + offsets[interval], every position compared with capacity.
//
// EX false: 4:4:4 with K.3 - K.6 (hhsr_jpeg_entropy: `comps` blocks per MCU, component = block index mod comps, the tables of
// d_huff).  EX true (hhsr_jpeg_entropy_ex): `comps` is the blocks per MCU of `layout`, the code words are the argument
// `codes`, and a symbol they do not have (entry 0) makes the write pass store UINT64_MAX over the length word.
template <bool EX>
struct ScanTables {};  // (EX false: nothing travels with the launch)
template <>
struct ScanTables<true> {
    uint32_t chroma;   // bit p: position p of an MCU codes with the chroma tables
    uint32_t dist;     // 4 bits per position: the DC prediction is the block that many blocks back
    uint64_t* length;  // the length word
    HuffCodes codes;   // 544 words, by value: no copy to enqueue, the call stays capturable
};
template <bool WRITE, bool EX>
__global__ void __launch_bounds__(64) k_jpeg_scan(const int16_t* __restrict__ coef, int comps, unsigned restart_mcus,
                                                   size_t n_mcu, size_t n_int, uint32_t* __restrict__ sizes,
                                                   const uint64_t* __restrict__ offsets, uint8_t* __restrict__ scan,
                                                   size_t capacity, ScanTables<EX> ex) {
    __shared__ uint32_t huff[HUFF_WORDS];
    __shared__ uint32_t bits[SCAN_WORDS];
    const int lane = threadIdx.x;
    const size_t it = blockIdx.x;
    if constexpr (EX) {
        for (int i = lane; i < HUFF_WORDS; i += 64) huff[i] = reinterpret_cast<const uint32_t*>(&ex.codes)[i];
    } else {
        for (int i = lane; i < HUFF_WORDS; i += 64) huff[i] = reinterpret_cast<const uint32_t*>(&d_huff)[i];
    }
    bool missing = false;  // (EX) a symbol without a code
    for (int i = lane; i < SCAN_WORDS; i += 64) bits[i] = 0;
    const uint32_t* dc_tab = huff;             // [2][16]
    const uint32_t* ac_tab = huff + 32;        // [2][256]
    const size_t mcu0 = it * restart_mcus;
    const size_t mcus = min((size_t)restart_mcus, n_mcu - mcu0);
    const unsigned nblk = (unsigned)mcus * comps;  // <= 65535 x 3
    const int16_t* __restrict__ base = coef + mcu0 * comps * 64;
    uint64_t pos = WRITE ? offsets[it] : 0;    // next output byte (WRITE) / bytes so far (SIZE)
    unsigned carry = 0;                        // bits of an unfinished byte, at the top of bits[0]
    __syncthreads();
    for (unsigned b0 = 0; b0 < nblk; b0 += 64) {
        const unsigned j = b0 + lane;
        const bool live = j < nblk;
        const int c = live ? (int)(j % comps) : 0;
        int tab = c ? 1 : 0, back = comps;
        if constexpr (EX) {
            tab = (int)(ex.chroma >> c & 1);
            back = (int)(ex.dist >> (4 * c) & 15);
        }
        const int16_t* __restrict__ blk = base + (size_t)(live ? j : 0) * 64;
        // DC prediction: the block of the same component before this one in the interval (4:4:4: in the previous MCU)
        const int pred = (live && j >= (unsigned)back) ? jpeg_clamp_coef(blk[-back * 64], true) : 0;
        int len = 0;
        if (live) {
            const bool bad = jpeg_code_block(blk, pred, dc_tab + tab * 16, ac_tab + tab * 256, [&](uint32_t, int n) { len += n; });
            if (EX && WRITE) missing |= bad;
        }
        int incl = len;  // inclusive wave prefix sum
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const unsigned total = carry + (unsigned)__shfl(incl, 63, 64);
        if (live) {
            const unsigned p0 = carry + (unsigned)(incl - len);
            unsigned wpos = p0 >> 5;
            int nacc = (int)(p0 & 31);
            uint64_t acc = 0;
            jpeg_code_block(blk, pred, dc_tab + tab * 16, ac_tab + tab * 256, [&](uint32_t v, int n) {
                acc |= (uint64_t)v << (64 - nacc - n);  // nacc < 32, n <= 26
                nacc += n;
                if (nacc >= 32) {
                    atomicOr(&bits[wpos], (uint32_t)(acc >> 32));
                    ++wpos;
                    acc <<= 32;
                    nacc -= 32;
                }
            });
            if (nacc > 0) atomicOr(&bits[wpos], (uint32_t)(acc >> 32));
        }
        __syncthreads();
        const bool last = b0 + 64 >= nblk;
        unsigned nbytes = total >> 3;
        unsigned rem = total & 7;
        if (last && rem) {  // pad the interval's last byte with 1-bits
            if (lane == 0) atomicOr(&bits[nbytes >> 2], (0xffu >> rem) << (24 - 8 * (nbytes & 3)));
            ++nbytes;
            rem = 0;
            __syncthreads();
        }
        for (unsigned k0 = 0; k0 < nbytes; k0 += 64) {
            const unsigned k = k0 + lane;
            const bool have = k < nbytes;
            const uint32_t byte = have ? (bits[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu : 0u;
            const unsigned long long ff = __ballot(have && byte == 0xffu);
            if (WRITE && have) {
                const uint64_t at = pos + lane + __popcll(ff & ((1ull << lane) - 1));  // (pos: behind the bytes before k0)
                if (at < capacity) scan[at] = (uint8_t)byte;
                if (byte == 0xffu && at + 1 < capacity) scan[at + 1] = 0;
            }
            pos += min(64u, nbytes - k0) + __popcll(ff);
            // (uniform: k0 and nbytes are)
        }
        const uint32_t carried = rem ? bits[nbytes >> 2] >> (24 - 8 * (nbytes & 3)) & 0xffu : 0u;
        __syncthreads();
        for (unsigned i = lane; i <= (total >> 5) && i < SCAN_WORDS; i += 64) bits[i] = 0;
        __syncthreads();
        if (lane == 0 && rem) bits[0] = carried << 24;
        carry = rem;
        __syncthreads();
    }
    const bool marker = it + 1 < n_int;
    if (WRITE) {
        if (marker && lane == 0) {
            if (pos < capacity) scan[pos] = 0xff;
            if (pos + 1 < capacity) scan[pos + 1] = (uint8_t)(0xd0 + (it & 7));
        }
        if constexpr (EX) {  // (every interval that finds one stores the same word, behind the scan of the sizes)
            if (__any(missing) && lane == 0) *ex.length = UINT64_MAX;
        }
    } else if (lane == 0) {
        sizes[it] = (uint32_t)(pos + (marker ? 2 : 0));  // <= 2 x 216 x 196605 + 2
    }
}

// Exclusive scan of sizes -> offsets in three steps: a total per group of SCAN_GROUP intervals, the groups' exclusive scan
// (one workgroup; it also writes the length word), then the offsets inside every group.
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* sm, uint64_t* total) {  // 256 threads
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    __syncthreads();
    if (lane == 63) sm[w] = incl;
    __syncthreads();
    uint64_t before = 0;
    for (int i = 0; i < w; ++i) before += sm[i];
    *total = sm[0] + sm[1] + sm[2] + sm[3];
    return before + incl - v;
}

__global__ void __launch_bounds__(256) k_jpeg_group_totals(const uint32_t* __restrict__ sizes, size_t n_int,
                                                            uint64_t* __restrict__ totals) {
    __shared__ uint64_t sm[4];
    const size_t i0 = (size_t)blockIdx.x * SCAN_GROUP + (size_t)threadIdx.x * (SCAN_GROUP / 256);
    uint64_t v = 0;
    for (int k = 0; k < SCAN_GROUP / 256; ++k) v += i0 + k < n_int ? sizes[i0 + k] : 0u;
    uint64_t total;
    block_excl_scan(v, sm, &total);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_jpeg_scan_groups(uint64_t* __restrict__ totals, size_t n_groups,
                                                           uint64_t* __restrict__ length) {
    __shared__ uint64_t sm[4];
    uint64_t run = 0;
    for (size_t g0 = 0; g0 < n_groups; g0 += 256) {  // (uniform trip count)
        const size_t g = g0 + threadIdx.x;
        const uint64_t v = g < n_groups ? totals[g] : 0;
        uint64_t total;
        const uint64_t ex = block_excl_scan(v, sm, &total);
        if (g < n_groups) totals[g] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) *length = run;
}

__global__ void __launch_bounds__(256) k_jpeg_offsets(const uint32_t* __restrict__ sizes, size_t n_int,
                                                       const uint64_t* __restrict__ totals, uint64_t* __restrict__ offsets) {
    __shared__ uint64_t sm[4];
    constexpr int PER = SCAN_GROUP / 256;
    const size_t i0 = (size_t)blockIdx.x * SCAN_GROUP + (size_t)threadIdx.x * PER;
    uint32_t s[PER];
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        s[k] = i0 + k < n_int ? sizes[i0 + k] : 0u;
        v += s[k];
    }
    uint64_t total;
    uint64_t at = totals[blockIdx.x] + block_excl_scan(v, sm, &total);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (i0 + k < n_int) offsets[i0 + k] = at;
        at += s[k];
    }
}

// The five launches of the entropy coder.  EX false: hhsr_jpeg_entropy's kernels, untouched by the extended route.
template <bool EX>
static void jpeg_entropy_launch(const int16_t* coef, const jpeg::Geom& g, int restart_mcus, void* scratch, uint8_t* scan,
                                size_t capacity, uint64_t* length, const ScanTables<EX>& ex, hipStream_t s) {
    uint64_t* offsets = (uint64_t*)scratch;
    uint64_t* totals = offsets + g.n_int;
    uint32_t* sizes = (uint32_t*)(totals + g.n_groups);
    const dim3 wave(64), wg(256), ints((unsigned)g.n_int), groups((unsigned)g.n_groups);  // n_int <= 2^26
    hipLaunchKernelGGL((k_jpeg_scan<false, EX>), ints, wave, 0, s, coef, g.bpm, (unsigned)restart_mcus, g.n_mcu, g.n_int,
                       sizes, (const uint64_t*)nullptr, (uint8_t*)nullptr, (size_t)0, ex);
    hipLaunchKernelGGL(k_jpeg_group_totals, groups, wg, 0, s, (const uint32_t*)sizes, g.n_int, totals);
    hipLaunchKernelGGL(k_jpeg_scan_groups, dim3(1), wg, 0, s, totals, g.n_groups, length);
    hipLaunchKernelGGL(k_jpeg_offsets, groups, wg, 0, s, (const uint32_t*)sizes, g.n_int, (const uint64_t*)totals, offsets);
    hipLaunchKernelGGL((k_jpeg_scan<true, EX>), ints, wave, 0, s, coef, g.bpm, (unsigned)restart_mcus, g.n_mcu, g.n_int,
                       sizes, (const uint64_t*)offsets, scan, capacity, ex);
}

// position -> tables and prediction distance of an MCU's blocks: Y Cb Cr (or Y alone) | Y Y Y Y Cb Cr
static inline void jpeg_layout(const jpeg::Geom& g, int subsampling, uint32_t* chroma, uint32_t* dist) {
    *chroma = subsampling ? 0x30u : 0x6u & ((1u << g.bpm) - 1);
    *dist = subsampling ? 0x661113u : (uint32_t)g.bpm * 0x111u;
}

extern "C" int hhsr_jpeg_entropy_ex(const int16_t* coef, int H, int W, int out_channels, int restart_mcus, int subsampling,
                                    const uint8_t* spec, void* scratch, size_t scratch_bytes, uint8_t* scan, size_t capacity,
                                    uint64_t* length, void* stream) {
    HHSR_ARG(coef != nullptr && scratch != nullptr && scan != nullptr && length != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    JPEG_ARG_SUB();
    HHSR_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)length & 7) == 0);
    const jpeg::Geom g = jpeg::geom(H, W, out_channels, restart_mcus, subsampling);
    HHSR_ARG(scratch_bytes >= g.scratch_bytes);
    HHSR_ARG(capacity <= SIZE_MAX - (uintptr_t)scan);
    HHSR_ARG(jpeg_disjoint(coef, g.coef_bytes, scratch, g.scratch_bytes) && jpeg_disjoint(coef, g.coef_bytes, scan, capacity) &&
             jpeg_disjoint(coef, g.coef_bytes, length, 8) && jpeg_disjoint(scratch, g.scratch_bytes, scan, capacity) &&
             jpeg_disjoint(scratch, g.scratch_bytes, length, 8) && jpeg_disjoint(scan, capacity, length, 8));
    HuffSpec store[4];
    const HuffSpec* specs[4];
    const bool spec_is_valid = jpeg::specs_from_abi(spec, out_channels == 1 ? 2 : 4, store, specs);
    HHSR_ARG(spec_is_valid);
    ScanTables<true> ex;
    jpeg_layout(g, subsampling, &ex.chroma, &ex.dist);
    ex.length = length;
    ex.codes = jpeg::huff_codes(specs);  // annex C, on the host
    jpeg_entropy_launch<true>(coef, g, restart_mcus, scratch, scan, capacity, length, ex, (hipStream_t)stream);
    HHSR_LAUNCHED();
}

extern "C" int hhsr_jpeg_entropy(const int16_t* coef, int H, int W, int out_channels, int restart_mcus, void* scratch,
                                 size_t scratch_bytes, uint8_t* scan, size_t capacity, uint64_t* length, void* stream) {
    HHSR_ARG(coef != nullptr && scratch != nullptr && scan != nullptr && length != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    HHSR_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)length & 7) == 0);
    const jpeg::Geom g = jpeg::geom(H, W, out_channels, restart_mcus);
    HHSR_ARG(scratch_bytes >= g.scratch_bytes);
    HHSR_ARG(capacity <= SIZE_MAX - (uintptr_t)scan);
    HHSR_ARG(jpeg_disjoint(coef, g.coef_bytes, scratch, g.scratch_bytes) && jpeg_disjoint(coef, g.coef_bytes, scan, capacity) &&
             jpeg_disjoint(coef, g.coef_bytes, length, 8) && jpeg_disjoint(scratch, g.scratch_bytes, scan, capacity) &&
             jpeg_disjoint(scratch, g.scratch_bytes, length, 8) && jpeg_disjoint(scan, capacity, length, 8));
    jpeg_entropy_launch<false>(coef, g, restart_mcus, scratch, scan, capacity, length, ScanTables<false>(), (hipStream_t)stream);
    HHSR_LAUNCHED();
}

// ---- symbol counts --------------------------------------------------------------------------------------------------------------
// A block's symbols need its own coefficients and one DC value before it, nothing of the interval's other blocks: a thread
// per block, a bounded number of persistent workgroups that stride over all blocks, counts in LDS [4][256] (DC luma, AC luma,
// DC chroma, AC chroma; a workgroup sees fewer than 2^32 symbols: at most 2^28 blocks over 512 workgroups), one partial
// table per workgroup, summed by a second launch.  Integer sums: the same counts whatever the order.
__global__ void __launch_bounds__(jpeg::HIST_THREADS) k_jpeg_histogram(const int16_t* __restrict__ coef, unsigned bpm,
                                                                        uint32_t chroma, uint32_t dist, unsigned restart_mcus,
                                                                        size_t n_blocks, uint64_t* __restrict__ partial) {
    __shared__ uint32_t cnt[4 * 256];
    const int t = threadIdx.x;
    for (int i = t; i < 4 * 256; i += jpeg::HIST_THREADS) cnt[i] = 0;
    __syncthreads();
    for (size_t b = (size_t)blockIdx.x * jpeg::HIST_THREADS + t; b < n_blocks; b += (size_t)gridDim.x * jpeg::HIST_THREADS) {
        const size_t mcu = b / bpm;
        const unsigned p = (unsigned)(b - mcu * bpm);
        const unsigned j = (unsigned)(mcu % restart_mcus) * bpm + p;  // the block's index in its interval
        const unsigned back = dist >> (4 * p) & 15;
        const int16_t* __restrict__ blk = coef + b * 64;
        const int pred = j >= back ? jpeg_clamp_coef(blk[-(int)back * 64], true) : 0;
        uint32_t* tab = cnt + (chroma >> p & 1) * 512;
        jpeg_walk_block(blk, pred, [&](bool is_ac, int s, int, int) { atomicAdd(&tab[(is_ac ? 256 : 0) + s], 1u); });
    }
    __syncthreads();
    for (int i = t; i < 4 * 256; i += jpeg::HIST_THREADS) partial[(size_t)blockIdx.x * 1024 + i] = cnt[i];
}

// 64 workgroups of 16 bins: 16 lanes read the bins of one partial table (128 consecutive bytes), the 16 groups of lanes
// take every 16th table, LDS adds the groups up.  (One thread per bin walking all tables alone is a chain of n_partial
// dependent-latency loads: measured 0.2 ms of the 0.27 ms of both launches at 48 MP.)
__global__ void __launch_bounds__(256) k_jpeg_histogram_sum(const uint64_t* __restrict__ partial, unsigned n_partial,
                                                             uint64_t* __restrict__ counts) {
    __shared__ uint64_t part[16][16];
    const unsigned bin = threadIdx.x & 15, slice = threadIdx.x >> 4;
    uint64_t sum = 0;
    for (unsigned g = slice; g < n_partial; g += 16) sum += partial[(size_t)g * 1024 + blockIdx.x * 16 + bin];
    part[slice][bin] = sum;
    __syncthreads();
    if (slice == 0) {
#pragma unroll
        for (int k = 1; k < 16; ++k) sum += part[k][bin];
        counts[blockIdx.x * 16 + bin] = sum;
    }
}

extern "C" int hhsr_jpeg_histogram(const int16_t* coef, int H, int W, int out_channels, int subsampling, int restart_mcus,
                                   uint64_t* counts, void* scratch, size_t scratch_bytes, void* stream) {
    HHSR_ARG(coef != nullptr && counts != nullptr && scratch != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    JPEG_ARG_SUB();
    HHSR_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)counts & 7) == 0);
    const jpeg::Geom g = jpeg::geom(H, W, out_channels, restart_mcus, subsampling);
    HHSR_ARG(scratch_bytes >= g.hist_bytes);
    HHSR_ARG(jpeg_disjoint(coef, g.coef_bytes, scratch, g.hist_bytes) && jpeg_disjoint(coef, g.coef_bytes, counts, jpeg::HIST_TABLE_BYTES) &&
             jpeg_disjoint(scratch, g.hist_bytes, counts, jpeg::HIST_TABLE_BYTES));
    uint32_t chroma, dist;
    jpeg_layout(g, subsampling, &chroma, &dist);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_jpeg_histogram, dim3((unsigned)g.hist_groups), dim3(jpeg::HIST_THREADS), 0, s, coef, (unsigned)g.bpm,
                       chroma, dist, (unsigned)restart_mcus, g.n_blocks, (uint64_t*)scratch);
    hipLaunchKernelGGL(k_jpeg_histogram_sum, dim3(64), dim3(256), 0, s, (const uint64_t*)scratch, (unsigned)g.hist_groups, counts);
    HHSR_LAUNCHED();
}
