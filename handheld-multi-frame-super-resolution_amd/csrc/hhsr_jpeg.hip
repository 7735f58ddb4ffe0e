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
#include "hhsr_common.h"

// ---- tables (T.81 annex K) ------------------------------------------------------------------------------------------------
namespace {
#define JPEG_ZIGZAG                                                                                                    \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,                          \
     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,                          \
     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
#define JPEG_K1_LUMA                                                                                                   \
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,       \
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,       \
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99}
#define JPEG_K2_CHROMA                                                                                                 \
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, \
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}
// (one text each for the host's header writer and the kernels: a host array cannot be indexed by a lane)
constexpr uint8_t ZIGZAG[64] = JPEG_ZIGZAG;  // ZIGZAG[k]: row-major index u * 8 + v of the k-th coefficient
constexpr uint8_t K1_LUMA[64] = JPEG_K1_LUMA;
constexpr uint8_t K2_CHROMA[64] = JPEG_K2_CHROMA;

struct HuffSpec {
    uint8_t bits[16];   // BITS: codes of length 1 .. 16
    int n;              // number of symbols
    uint8_t vals[162];  // HUFFVAL
};
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// The device's code tables, made from the four specifications at compile time (annex C): entry = code | length << 16, a
// symbol the table does not have = 0.  [0] luma, [1] chroma; DC symbols are the 12 categories, AC symbols run << 4 | size.
struct HuffCodes {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr void huff_fill(const HuffSpec& s, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) out[s.vals[k++]] = code++ | ((uint32_t)len << 16);
        code <<= 1;
    }
}
constexpr HuffCodes huff_codes() {
    HuffCodes h = {};
    huff_fill(DC_LUMA, h.dc[0]);
    huff_fill(DC_CHROMA, h.dc[1]);
    huff_fill(AC_LUMA, h.ac[0]);
    huff_fill(AC_CHROMA, h.ac[1]);
    return h;
}
constexpr int HUFF_WORDS = sizeof(HuffCodes) / 4;  // 544
}  // namespace

__device__ const HuffCodes d_huff = huff_codes();
__device__ const uint8_t d_zigzag[64] = JPEG_ZIGZAG;
__device__ const uint8_t d_base_q[2][64] = {JPEG_K1_LUMA, JPEG_K2_CHROMA};

// IJG quality scaling: the percentage s, then a table entry
static inline int jpeg_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
__host__ __device__ static inline int jpeg_q(int base, int scale) {
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// ---- geometry shared by the four entry points ----------------------------------------------------------------------------
constexpr int JPEG_MAX_DIM = 65535;
constexpr int SCAN_GROUP = 2048;          // intervals per workgroup of the offset scan
constexpr size_t BLOCK_MAX_BYTES = 216;   // 64 coefficients x (16-bit code + 11 magnitude bits) / 8
struct JpegGeom {
    int mcux, mcuy;
    size_t n_mcu, n_int, n_groups;
    size_t coef_bytes, scratch_bytes, max_scan;
};
static inline JpegGeom jpeg_geom(int H, int W, int comps, int restart_mcus) {
    JpegGeom g;
    g.mcux = (W + 7) / 8;
    g.mcuy = (H + 7) / 8;
    g.n_mcu = (size_t)g.mcux * g.mcuy;  // <= 8192^2
    g.n_int = (g.n_mcu + restart_mcus - 1) / restart_mcus;
    g.n_groups = (g.n_int + SCAN_GROUP - 1) / SCAN_GROUP;
    g.coef_bytes = g.n_mcu * comps * 64 * sizeof(int16_t);
    // scratch: uint64 offsets[n_int] | uint64 group totals[n_groups] | uint32 sizes[n_int]
    g.scratch_bytes = (g.n_int + g.n_groups) * sizeof(uint64_t) + g.n_int * sizeof(uint32_t);
    g.max_scan = 2 * BLOCK_MAX_BYTES * g.n_mcu * comps + 2 * (g.n_int - 1);
    return g;
}
#define JPEG_ARG_DIMS() \
    HHSR_ARG(H > 0 && W > 0 && H <= JPEG_MAX_DIM && W <= JPEG_MAX_DIM)

// ---- header (host only) -----------------------------------------------------------------------------------------------------
extern "C" int hhsr_jpeg_header(int H, int W, int out_channels, int quality, int restart_mcus, uint8_t* out,
                                size_t out_capacity, size_t* length) {
    HHSR_ARG(out != nullptr && length != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(quality >= 1 && quality <= 100);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    const int nc = out_channels;
    const JpegGeom g = jpeg_geom(H, W, nc, restart_mcus);
    const bool dri = (size_t)restart_mcus < g.n_mcu;
    const HuffSpec* specs[4] = {&DC_LUMA, &AC_LUMA, &DC_CHROMA, &AC_CHROMA};
    const int ntab = nc == 1 ? 1 : 2;
    size_t need = 2 + 18 + (size_t)ntab * 69 + (10 + 3 * nc) + (dri ? 6 : 0) + (8 + 2 * nc);
    for (int t = 0; t < 2 * ntab; ++t) need += 21 + specs[t]->n;
    *length = need;
    HHSR_ARG(out_capacity >= need);
    uint8_t* p = out;
    auto u8 = [&](int v) { *p++ = (uint8_t)v; };
    auto u16 = [&](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
    u16(0xFFD8);
    u16(0xFFE0); u16(16);  // APP0: JFIF 1.02, no units, aspect 1:1, no thumbnail
    for (const char c : {'J', 'F', 'I', 'F', '\0'}) u8(c);
    u8(1); u8(2); u8(0); u16(1); u16(1); u8(0); u8(0);
    const int scale = jpeg_scale(quality);
    for (int t = 0; t < ntab; ++t) {
        u16(0xFFDB); u16(67); u8(t);
        for (int k = 0; k < 64; ++k) u8(jpeg_q((t ? K2_CHROMA : K1_LUMA)[ZIGZAG[k]], scale));
    }
    u16(0xFFC0); u16(8 + 3 * nc); u8(8); u16(H); u16(W); u8(nc);
    for (int c = 0; c < nc; ++c) { u8(c + 1); u8(0x11); u8(c ? 1 : 0); }
    for (int t = 0; t < 2 * ntab; ++t) {
        const HuffSpec& s = *specs[t];
        u16(0xFFC4); u16(19 + s.n); u8(((t & 1) << 4) | (t >> 1));
        for (int i = 0; i < 16; ++i) u8(s.bits[i]);
        for (int i = 0; i < s.n; ++i) u8(s.vals[i]);
    }
    if (dri) { u16(0xFFDD); u16(4); u16(restart_mcus); }
    u16(0xFFDA); u16(6 + 2 * nc); u8(nc);
    for (int c = 0; c < nc; ++c) { u8(c + 1); u8(c ? 0x11 : 0x00); }
    u8(0); u8(63); u8(0);
    if ((size_t)(p - out) != need) {
        hhsr_set_error("hhsr_jpeg_header: internal length mismatch");
        return -2;
    }
    return 0;
}

extern "C" int hhsr_jpeg_workspace(int H, int W, int out_channels, int restart_mcus, size_t* coef_bytes,
                                   size_t* scratch_bytes, size_t* max_scan_bytes) {
    HHSR_ARG(coef_bytes != nullptr && scratch_bytes != nullptr && max_scan_bytes != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    const JpegGeom g = jpeg_geom(H, W, out_channels, restart_mcus);
    *coef_bytes = g.coef_bytes;
    *scratch_bytes = g.scratch_bytes;
    *max_scan_bytes = g.max_scan;
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
    if (t < 64 * (NC == 1 ? 1 : 2)) Q[t >> 6][t & 63] = (float)jpeg_q(d_base_q[t >> 6][t & 63], scale);
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
    for (int i = t; i < NC * 256; i += 256) {  // row passes: (component, row, block)
        float* row = &P[i >> 8][(i >> 5) & 7][(i & 31) * 8];
        float4 a = reinterpret_cast<float4*>(row)[0], b = reinterpret_cast<float4*>(row)[1];
        float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        dct8(x);
        reinterpret_cast<float4*>(row)[0] = make_float4(x[0], x[1], x[2], x[3]);
        reinterpret_cast<float4*>(row)[1] = make_float4(x[4], x[5], x[6], x[7]);
    }
    __syncthreads();
#pragma unroll
    for (int i = t; i < NC * 256; i += 256) {  // column passes: (component, block, column), then the division
        const int c = i >> 8, col = i & 255, b = col >> 3, v = col & 7;
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = P[c][u][col];
        dct8(x);
        int16_t* o = &O[(b * NC + c) * 64];
        const float* q = Q[c ? 1 : 0];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = u * 8 + v;
            const float lo = k == 0 ? -1024.f : -1023.f;
            o[zpos[k]] = (int16_t)fminf(fmaxf(rintf(x[u] / q[k]), lo), 1023.f);
        }
    }
    __syncthreads();
    const int nvalid = min(DCT_MCUS, mcux - bx0);  // MCUs of this workgroup that exist
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(coef + ((size_t)by * mcux + bx0) * (NC * 64));
    for (int i = t; i < nvalid * NC * 8; i += 256) dst[i] = reinterpret_cast<const uint4*>(O)[i];
}

static inline bool jpeg_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}

extern "C" int hhsr_jpeg_dct(const float* image, int H, int W, int channels, int out_channels, int quality, int16_t* coef,
                             size_t coef_bytes, void* stream) {
    HHSR_ARG(image != nullptr && coef != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(channels == 1 || channels == 3);
    HHSR_ARG(out_channels == channels || out_channels == 1);
    HHSR_ARG(quality >= 1 && quality <= 100);
    HHSR_ARG(((uintptr_t)image & 3) == 0 && ((uintptr_t)coef & 15) == 0);
    const JpegGeom g = jpeg_geom(H, W, out_channels, 1);
    HHSR_ARG(coef_bytes >= g.coef_bytes);
    HHSR_ARG(jpeg_disjoint(image, (size_t)H * W * channels * sizeof(float), coef, g.coef_bytes));
    const dim3 grid((unsigned)hhsr_cdiv(g.mcux, DCT_MCUS), (unsigned)g.mcuy), block(256);
    const int scale = jpeg_scale(quality);
#define HHSR_JPEG_DCT(NC, STEP) \
    hipLaunchKernelGGL((k_jpeg_dct<NC, STEP>), grid, block, 0, (hipStream_t)stream, image, H, W, g.mcux, scale, coef)
    if (out_channels == 3) HHSR_JPEG_DCT(3, 3);
    else if (channels == 3) HHSR_JPEG_DCT(1, 3);
    else HHSR_JPEG_DCT(1, 1);
#undef HHSR_JPEG_DCT
    HHSR_LAUNCHED();
}

// ---- entropy coding -----------------------------------------------------------------------------------------------------------
// Bits of a wave's 64 blocks: at most 7 carried bits + 64 x (22 DC + 63 x 26 AC) = 106247 bits = 3321 words.
constexpr int SCAN_WORDS = 3328;

__device__ __forceinline__ int jpeg_clamp_coef(int v, bool dc) { return max(dc ? -1024 : -1023, min(v, 1023)); }

// A block's bit string, symbol by symbol, through put(bits, count): count <= 26, bits < 2^count.
template <typename Put>
__device__ __forceinline__ void jpeg_code_block(const int16_t* __restrict__ blk, int pred, const uint32_t* __restrict__ dc,
                                                const uint32_t* __restrict__ ac, Put put) {
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 w = reinterpret_cast<const uint4*>(blk)[g];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int raw = (int)(int16_t)(ws[j >> 1] >> ((j & 1) * 16));
            if (g == 0 && j == 0) {
                const int d = jpeg_clamp_coef(raw, true) - pred;       // |d| <= 2047: category <= 11
                const int cat = 32 - __clz(abs(d));
                const uint32_t e = dc[cat];                             // cat <= 11 < 16
                put((e & 0xffffu) << cat | (uint32_t)((d < 0 ? d - 1 : d) & ((1 << cat) - 1)), (int)(e >> 16) + cat);
            } else {
                const int v = jpeg_clamp_coef(raw, false);             // |v| <= 1023: size <= 10
                if (v == 0) {
                    ++run;
                } else {
                    while (run >= 16) {
                        const uint32_t z = ac[0xF0];
                        put(z & 0xffffu, (int)(z >> 16));
                        run -= 16;
                    }
                    const int cat = 32 - __clz(abs(v));
                    const uint32_t e = ac[(run << 4) | cat];            // run <= 15, cat <= 10: < 256
                    put((e & 0xffffu) << cat | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << cat) - 1)), (int)(e >> 16) + cat);
                    run = 0;
                }
            }
        }
    }
    if (run) put(ac[0] & 0xffffu, (int)(ac[0] >> 16));  // EOB
}

// One wave per restart interval.  WRITE false: sizes[interval] = its bytes (stuffing, padding and RSTm included).
// WRITE true: the bytes to scan + offsets[interval], every position compared with capacity.
template <bool WRITE>
__global__ void __launch_bounds__(64) k_jpeg_scan(const int16_t* __restrict__ coef, int comps, unsigned restart_mcus,
                                                   size_t n_mcu, size_t n_int, uint32_t* __restrict__ sizes,
                                                   const uint64_t* __restrict__ offsets, uint8_t* __restrict__ scan,
                                                   size_t capacity) {
    __shared__ uint32_t huff[HUFF_WORDS];
    __shared__ uint32_t bits[SCAN_WORDS];
    const int lane = threadIdx.x;
    const size_t it = blockIdx.x;
    for (int i = lane; i < HUFF_WORDS; i += 64) huff[i] = reinterpret_cast<const uint32_t*>(&d_huff)[i];
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
        const int c = live ? (int)(j % comps) : 0, tab = c ? 1 : 0;
        const int16_t* __restrict__ blk = base + (size_t)(live ? j : 0) * 64;
        // DC prediction: the same component of the previous MCU of this interval
        const int pred = (live && j >= (unsigned)comps) ? jpeg_clamp_coef(blk[-comps * 64], true) : 0;
        int len = 0;
        if (live) jpeg_code_block(blk, pred, dc_tab + tab * 16, ac_tab + tab * 256, [&](uint32_t, int n) { len += n; });
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

extern "C" int hhsr_jpeg_entropy(const int16_t* coef, int H, int W, int out_channels, int restart_mcus, void* scratch,
                                 size_t scratch_bytes, uint8_t* scan, size_t capacity, uint64_t* length, void* stream) {
    HHSR_ARG(coef != nullptr && scratch != nullptr && scan != nullptr && length != nullptr);
    JPEG_ARG_DIMS();
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(restart_mcus >= 1 && restart_mcus <= 65535);
    HHSR_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)length & 7) == 0);
    const JpegGeom g = jpeg_geom(H, W, out_channels, restart_mcus);
    HHSR_ARG(scratch_bytes >= g.scratch_bytes);
    HHSR_ARG(capacity <= SIZE_MAX - (uintptr_t)scan);
    HHSR_ARG(jpeg_disjoint(coef, g.coef_bytes, scratch, g.scratch_bytes) && jpeg_disjoint(coef, g.coef_bytes, scan, capacity) &&
             jpeg_disjoint(coef, g.coef_bytes, length, 8) && jpeg_disjoint(scratch, g.scratch_bytes, scan, capacity) &&
             jpeg_disjoint(scratch, g.scratch_bytes, length, 8) && jpeg_disjoint(scan, capacity, length, 8));
    uint64_t* offsets = (uint64_t*)scratch;
    uint64_t* totals = offsets + g.n_int;
    uint32_t* sizes = (uint32_t*)(totals + g.n_groups);
    hipStream_t s = (hipStream_t)stream;
    const dim3 wave(64), wg(256), ints((unsigned)g.n_int), groups((unsigned)g.n_groups);  // n_int <= 2^26
    hipLaunchKernelGGL(k_jpeg_scan<false>, ints, wave, 0, s, coef, out_channels, (unsigned)restart_mcus, g.n_mcu, g.n_int,
                       sizes, (const uint64_t*)nullptr, (uint8_t*)nullptr, (size_t)0);
    hipLaunchKernelGGL(k_jpeg_group_totals, groups, wg, 0, s, (const uint32_t*)sizes, g.n_int, totals);
    hipLaunchKernelGGL(k_jpeg_scan_groups, dim3(1), wg, 0, s, totals, g.n_groups, length);
    hipLaunchKernelGGL(k_jpeg_offsets, groups, wg, 0, s, (const uint32_t*)sizes, g.n_int, (const uint64_t*)totals, offsets);
    hipLaunchKernelGGL(k_jpeg_scan<true>, ints, wave, 0, s, coef, out_channels, (unsigned)restart_mcus, g.n_mcu, g.n_int,
                       sizes, (const uint64_t*)offsets, scan, capacity);
    HHSR_LAUNCHED();
}
