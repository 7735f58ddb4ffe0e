// PNG output (include/hhsr.h "PNG output"): the finished float32 image -> the IDAT payload of a PNG file, both stages on the
// device, so that what crosses the host link is the file and not its samples.  The reference writes its PNG on the host
// (run_handheld.py: imsave) after the float32 image crossed the link.
//
// k_png_filter  quantises (the rule of hhsr_encode_image), filters (PNG 9: None, Sub, Up, Average, Paeth, or libpng's
//               adaptive choice per row) and counts the 256 byte values of the filtered stream.  12 B in + 3 or 6 B out
//               per RGB pixel: bandwidth-shaped.  A workgroup takes a row at a time, in segments of 4096 samples: the
//               segment of the row and of the row above are quantised into LDS (16-byte loads where the image allows
//               them), every thread filters four consecutive bytes read from LDS as dwords, the filtered bytes cross LDS
//               once more and leave as 16-byte stores.  The adaptive choice needs the whole row's five sums before the first byte can
//               be stored: a row of one segment is filtered from the LDS copy that was summed, a longer row is staged
//               a second time (192 KB of floats per 8000-pixel RGB row pair: from L2).  Counts: LDS atomics per
//               workgroup, one partial table per workgroup, summed by k_png_counts_sum — integers, no device atomics.
// k_png_size    one wave per interval: the bits of its dynamic-Huffman block (sum of code lengths) -> its bytes, and the
//               interval's two Adler-32 sums.
// (offsets)     the exclusive scan of the sizes: the three kernels of hhsr_jpeg.hip (hhsr_scan.h).
// k_png_write   one wave per interval, 1024 stream bytes at a time, 16 per lane: a lane sums the lengths of its codes, a
//               wave prefix sum places it, it ORs its codes into the wave's LDS bit buffer (LSB first; OR commutes), and
//               the wave stores the finished 32-bit words at their final place, every position compared with the
//               capacity.  The CRC-32 of the interval's bytes rides along: lane l owns the words l, l + 64, ... of the
//               interval and advances its remainder by 256 bytes per word with four table look-ups (x^2048 mod P);
//               at the end of the interval the lanes' remainders are aligned and XORed.
// k_png_finish  the CRC-32 of the whole stream and the Adler-32 of the filtered stream from the intervals' records:
//               both are plain sums of per-interval terms (remainder x x^(8 bytes behind it); s2 + s1 x bytes behind it).
#include "hhsr_common.h"
#include "hhsr_png_tables.h"
#include "hhsr_scan.h"
#include "hhsr_jpeg_tables.h"

static_assert(png::SCAN_GROUP == jpeg::SCAN_GROUP, "the offsets scan of hhsr_jpeg.hip works on groups of jpeg::SCAN_GROUP");

__device__ const png::CrcStride d_crc_stride = png::crc_stride();
__device__ const png::CrcPowers d_crc_powers = png::crc_powers();

static inline bool png_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}

#define PNG_ARG_FORMAT()                                     \
    HHSR_ARG(H > 0 && W > 0);                                \
    HHSR_ARG(out_channels == 1 || out_channels == 3);        \
    HHSR_ARG(bits == 8 || bits == 16);                       \
    HHSR_ARG(interval_bytes >= 1 && (uint32_t)interval_bytes <= png::MAX_INTERVAL)

// ---- workspace, code construction, the file's fixed parts (host only) ----------------------------------------------------------
extern "C" int hhsr_png_workspace(int H, int W, int out_channels, int bits, int interval_bytes, size_t* stream_bytes,
                                  size_t* scratch_bytes, size_t* max_deflate_bytes) {
    HHSR_ARG(stream_bytes != nullptr && scratch_bytes != nullptr && max_deflate_bytes != nullptr);
    PNG_ARG_FORMAT();
    png::Geom g;
    const bool fits_one_idat = png::geom(H, W, out_channels, bits, (uint32_t)interval_bytes, &g);
    HHSR_ARG(fits_one_idat /* the bound of the deflate stream <= 2^31 - 1 */);
    *stream_bytes = g.stream_bytes;
    *scratch_bytes = g.scratch_bytes;
    *max_deflate_bytes = g.max_deflate;
    return 0;
}

extern "C" int hhsr_png_huffman(const uint64_t* counts, uint8_t* spec) {
    HHSR_ARG(counts != nullptr && spec != nullptr);
    HHSR_ARG(((uintptr_t)counts & 7) == 0);
    HHSR_ARG(png_disjoint(counts, png::N_SYM * sizeof(uint64_t), spec, png::SPEC_BYTES));
    uint8_t built[png::SPEC_BYTES];
    const bool counts_are_usable = png::build_spec(counts, built);
    HHSR_ARG(counts_are_usable /* the end symbol and a byte value counted, the sum below 2^59 */);
    for (int i = 0; i < png::SPEC_BYTES; ++i) spec[i] = built[i];
    return 0;
}

extern "C" int hhsr_png_crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b, uint32_t* crc) {
    HHSR_ARG(crc != nullptr);
    *crc = png::crc_combine(crc_a, crc_b, len_b);
    return 0;
}

extern "C" int hhsr_png_file_head(int H, int W, int out_channels, int bits, uint64_t deflate_len, uint8_t* buf, size_t capacity,
                                  size_t* length) {
    HHSR_ARG(buf != nullptr && length != nullptr);
    HHSR_ARG(H > 0 && W > 0);
    HHSR_ARG(out_channels == 1 || out_channels == 3);
    HHSR_ARG(bits == 8 || bits == 16);
    HHSR_ARG(deflate_len >= 1 && deflate_len <= 0x7fffffffull - 6);  // one IDAT chunk: a 31-bit length
    *length = png::HEAD_BYTES;
    HHSR_ARG(capacity >= png::HEAD_BYTES);
    png::file_head(H, W, out_channels, bits, (uint32_t)deflate_len, buf);
    return 0;
}

extern "C" int hhsr_png_file_tail(uint32_t deflate_crc, uint64_t deflate_len, uint32_t adler, uint8_t* buf, size_t capacity,
                                  size_t* length) {
    HHSR_ARG(buf != nullptr && length != nullptr);
    HHSR_ARG(deflate_len >= 1 && deflate_len <= 0x7fffffffull - 6);
    *length = png::TAIL_BYTES;
    HHSR_ARG(capacity >= png::TAIL_BYTES);
    png::file_tail(deflate_crc, deflate_len, adler, buf);
    return 0;
}

// ---- quantise, filter, count ------------------------------------------------------------------------------------------------------
constexpr int PF_THREADS = 256;
constexpr int PF_SAMPLES = 4096;  // samples of a row a workgroup holds at a time (a whole number of pixels of them is used)
constexpr int PF_HALO = 16;       // LDS bytes in front of a segment: the pixel to its left (at most 6 bytes)

__device__ __forceinline__ float png_sample(float x, float M) {  // hhsr_encode_image's rule
    x = x == x ? x : 0.f;
    x = fminf(fmaxf(x, 0.f), 1.f);
    return rintf(x * M);
}

// sample i of a segment -> its 1 or 2 bytes (big-endian) at dst + i * BPS; dst is 2-byte aligned, i may be negative
template <int BPS>
__device__ __forceinline__ void png_put(uint8_t* dst, int i, float x, float M) {
    const uint32_t q = (uint32_t)png_sample(x, M);
    if constexpr (BPS == 1) dst[i] = (uint8_t)q;
    else *reinterpret_cast<uint16_t*>(dst + 2 * i) = (uint16_t)((q >> 8) | ((q & 0xffu) << 8));
}

// Samples [qs, q1) of a row -> dst[(q - q0) * BPS ...]; sample q is image[row0 + q * STEP] (STEP 3: channel 0 of RGB).
// zero: the row above row 0.  qs == q0 (no pixel to the left): the halo is zeroed.  vec: the image is 16-byte aligned.
template <int BPS, int STEP>
__device__ __forceinline__ void png_stage(const float* __restrict__ image, size_t row0, bool zero, bool vec, int qs, int q1,
                                          int q0, uint8_t* dst, float M) {
    const int t = threadIdx.x;
    if (qs == q0 && t < PF_HALO) dst[t - PF_HALO] = 0;
    if (zero) {
        for (int q = qs + t; q < q1; q += PF_THREADS) png_put<BPS>(dst, q - q0, 0.f, M);
        return;
    }
    if (STEP == 1 && vec) {  // float4 at 16-byte aligned indices; the pieces that stick out of [f0, f1) float by float
        const size_t f0 = row0 + (size_t)qs, f1 = row0 + (size_t)q1;
        for (size_t f = (f0 & ~(size_t)3) + 4 * (size_t)t; f < f1; f += 4 * PF_THREADS) {
            const int i = (int)((int64_t)f - (int64_t)row0) - q0;
            if (f >= f0 && f + 4 <= f1) {
                const float4 v = *reinterpret_cast<const float4*>(image + f);
                png_put<BPS>(dst, i, v.x, M);
                png_put<BPS>(dst, i + 1, v.y, M);
                png_put<BPS>(dst, i + 2, v.z, M);
                png_put<BPS>(dst, i + 3, v.w, M);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (f + k >= f0 && f + k < f1) png_put<BPS>(dst, i + k, image[f + k], M);
            }
        }
    } else {
        for (int q = qs + t; q < q1; q += PF_THREADS) png_put<BPS>(dst, q - q0, image[row0 + (size_t)q * STEP], M);
    }
}

// the five filtered values of a byte x with a to its left, b above, c above-left (PNG 9.2, 9.4)
__device__ __forceinline__ void png_candidates(int x, int a, int b, int c, int* v) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    v[0] = x;
    v[1] = (x - a) & 255;
    v[2] = (x - b) & 255;
    v[3] = (x - ((a + b) >> 1)) & 255;
    v[4] = (x - paeth) & 255;
}

// bytes [j, j + 4) of a staged row and the four bytes bpp to their left, as dwords (j a multiple of 4; bpp 1, 2, 3 or 6)
__device__ __forceinline__ void png_quad(const uint8_t* row, int j, int bpp, uint32_t* x, uint32_t* left) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(row + j);
    const uint32_t x0 = w[0], x1 = w[-1];
    *x = x0;
    if (bpp < 4) {
        *left = (x0 << (8 * bpp)) | (x1 >> (32 - 8 * bpp));
    } else {
        *left = (x1 << (8 * (bpp - 4))) | (w[-2] >> (32 - 8 * (bpp - 4)));
    }
}

// byte k of the quads x (this row), a (left), b (above), c (above-left) under the five filters
__device__ __forceinline__ void png_quad_candidates(uint32_t x, uint32_t a, uint32_t b, uint32_t c, int k, int* v) {
    png_candidates((int)(x >> (8 * k) & 255u), (int)(a >> (8 * k) & 255u), (int)(b >> (8 * k) & 255u), (int)(c >> (8 * k) & 255u), v);
}

template <int BPS, int STEP>
__global__ void __launch_bounds__(PF_THREADS) k_png_filter(const float* __restrict__ image, int H, int W, int och, int filter,
                                                            bool vec, uint8_t* __restrict__ filtered,
                                                            uint32_t* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) uint8_t cur_s[PF_HALO + PF_SAMPLES * BPS];
    __shared__ __attribute__((aligned(16))) uint8_t prev_s[PF_HALO + PF_SAMPLES * BPS];
    __shared__ __attribute__((aligned(16))) uint8_t fout[PF_SAMPLES * BPS + 32];
    __shared__ uint32_t cnt[256];
    __shared__ uint64_t red[PF_THREADS / 64][5];
    const int t = threadIdx.x;
    uint8_t* cur = cur_s + PF_HALO;
    uint8_t* prev = prev_s + PF_HALO;
    const int bpp = och * BPS;
    const size_t R = (size_t)W * bpp;              // bytes of a row without its filter type
    const size_t row_floats = (size_t)W * och * STEP;
    const int seg_pix = PF_SAMPLES / och;
    const int nseg = (W + seg_pix - 1) / seg_pix;
    const float M = BPS == 1 ? 255.f : 65535.f;
    cnt[t] = 0;
    __syncthreads();
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
        const size_t row0 = (size_t)y * row_floats;
        auto stage = [&](int seg) {  // the segment of this row and of the row above, each with the pixel to its left
            const int p0 = seg * seg_pix, p1 = min(W, p0 + seg_pix);
            const int q0 = p0 * och, qs = p0 ? q0 - och : q0, q1 = p1 * och;
            png_stage<BPS, STEP>(image, row0, false, vec, qs, q1, q0, cur, M);
            png_stage<BPS, STEP>(image, y ? row0 - row_floats : 0, y == 0, vec, qs, q1, q0, prev, M);
            return (q1 - q0) * BPS;  // the segment's bytes
        };
        int ftype = filter;
        if (filter == 5) {  // libpng's heuristic: the least sum of min(v, 256 - v); ties to the lowest type
            uint32_t s[5] = {0, 0, 0, 0, 0};  // (a thread sees at most R / 256 + 1 bytes of at most 128 each: R < 2^31)
            for (int seg = 0; seg < nseg; ++seg) {
                const int n = stage(seg);
                __syncthreads();
                for (int j = 4 * t; j < n; j += 4 * PF_THREADS) {  // four bytes per thread: LDS is read in dwords
                    uint32_t x, a, b, c;
                    png_quad(cur, j, bpp, &x, &a);
                    png_quad(prev, j, bpp, &b, &c);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (j + q < n) {
                            int v[5];
                            png_quad_candidates(x, a, b, c, q, v);
#pragma unroll
                            for (int k = 0; k < 5; ++k) s[k] += (uint32_t)(v[k] < 128 ? v[k] : 256 - v[k]);
                        }
                    }
                }
                if (nseg > 1) __syncthreads();  // (uniform) the next segment overwrites what is being read
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                uint64_t w = s[k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) w += __shfl_down(w, o, 64);
                if ((t & 63) == 0) red[t >> 6][k] = w;
            }
            __syncthreads();
            uint64_t best = 0;
            ftype = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                uint64_t w = 0;
                for (int i = 0; i < PF_THREADS / 64; ++i) w += red[i][k];
                if (k == 0 || w < best) best = w, ftype = k;
            }
        }
        for (int seg = 0; seg < nseg; ++seg) {
            int n;
            if (filter == 5 && nseg == 1) {
                n = (int)R;  // what the sums were taken of is still in LDS
            } else {
                n = stage(seg);
                __syncthreads();
            }
            const int lead = seg == 0 ? 1 : 0;  // the row's filter type goes in front of its first segment
            const size_t g0 = (size_t)y * (1 + R) + (seg == 0 ? 0 : 1 + (size_t)seg * seg_pix * bpp);
            const int mis = (int)(g0 & 15);     // fout[i] is byte g0 - mis + i of the stream: 16-byte pieces line up
            if (lead && t == 0) {
                fout[mis] = (uint8_t)ftype;
                atomicAdd(&cnt[ftype], 1u);
            }
            for (int j = 4 * t; j < n; j += 4 * PF_THREADS) {
                uint32_t x, a, b, c;
                png_quad(cur, j, bpp, &x, &a);
                png_quad(prev, j, bpp, &b, &c);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (j + q < n) {
                        int v[5];
                        png_quad_candidates(x, a, b, c, q, v);
                        const int f = ftype == 0 ? v[0] : ftype == 1 ? v[1] : ftype == 2 ? v[2] : ftype == 3 ? v[3] : v[4];
                        fout[mis + lead + j + q] = (uint8_t)f;
                        atomicAdd(&cnt[f], 1u);
                    }
                }
            }
            __syncthreads();
            const int i_end = mis + lead + n;
            uint8_t* __restrict__ dst = filtered + (g0 - mis);
            for (int i0 = 16 * t; i0 < i_end; i0 += 16 * PF_THREADS) {
                if (i0 >= mis && i0 + 16 <= i_end) {
                    *reinterpret_cast<uint4*>(dst + i0) = *reinterpret_cast<const uint4*>(fout + i0);
                } else {
                    for (int i = max(i0, mis); i < min(i0 + 16, i_end); ++i) dst[i] = fout[i];
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    partial[(size_t)blockIdx.x * 256 + t] = cnt[t];  // (a workgroup counts fewer than 2^31 bytes)
}

// 16 workgroups of 16 bins: 16 lanes read the bins of one partial table, the 16 groups of lanes take every 16th table, LDS
// adds the groups up (the shape of k_jpeg_histogram_sum)
__global__ void __launch_bounds__(256) k_png_counts_sum(const uint32_t* __restrict__ partial, unsigned n_partial,
                                                         uint64_t* __restrict__ counts) {
    __shared__ uint64_t part[16][16];
    const unsigned bin = threadIdx.x & 15, slice = threadIdx.x >> 4;
    uint64_t sum = 0;
    for (unsigned g = slice; g < n_partial; g += 16) sum += partial[(size_t)g * 256 + blockIdx.x * 16 + bin];
    part[slice][bin] = sum;
    __syncthreads();
    if (slice == 0) {
#pragma unroll
        for (int k = 1; k < 16; ++k) sum += part[k][bin];
        counts[blockIdx.x * 16 + bin] = sum;
    }
}

extern "C" int hhsr_png_filter(const float* image, int H, int W, int channels, int out_channels, int bits, int filter,
                               uint8_t* filtered, size_t filtered_bytes, uint64_t* counts, void* scratch, size_t scratch_bytes,
                               void* stream) {
    HHSR_ARG(image != nullptr && filtered != nullptr && counts != nullptr && scratch != nullptr);
    HHSR_ARG(H > 0 && W > 0);
    HHSR_ARG(channels == 1 || channels == 3);
    HHSR_ARG(out_channels == channels || out_channels == 1);
    HHSR_ARG(bits == 8 || bits == 16);
    HHSR_ARG(filter >= 0 && filter <= 5);
    png::Geom g;
    const bool fits_one_idat = png::geom(H, W, out_channels, bits, png::MAX_INTERVAL, &g);
    HHSR_ARG(fits_one_idat);
    HHSR_ARG(filtered_bytes >= g.stream_bytes && scratch_bytes >= g.scratch_filter);
    HHSR_ARG(((uintptr_t)image & 3) == 0 && ((uintptr_t)filtered & 15) == 0 && ((uintptr_t)counts & 7) == 0 &&
             ((uintptr_t)scratch & 7) == 0);
    const size_t image_bytes = (size_t)H * W * channels * sizeof(float);  // (H W bpp < 2^31: no overflow)
    HHSR_ARG(png_disjoint(image, image_bytes, filtered, g.stream_bytes) && png_disjoint(image, image_bytes, counts, 2048) &&
             png_disjoint(image, image_bytes, scratch, g.scratch_filter) && png_disjoint(filtered, g.stream_bytes, counts, 2048) &&
             png_disjoint(filtered, g.stream_bytes, scratch, g.scratch_filter) && png_disjoint(counts, 2048, scratch, g.scratch_filter));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)g.filter_groups), block(PF_THREADS);
    const bool vec = ((uintptr_t)image & 15) == 0;
#define HHSR_PNG_FILTER(BPS, STEP)                                                                                          \
    hipLaunchKernelGGL((k_png_filter<BPS, STEP>), grid, block, 0, s, image, H, W, out_channels, filter, vec, filtered,      \
                       (uint32_t*)scratch)
    const bool strided = out_channels != channels;
    if (bits == 8) {
        if (strided) HHSR_PNG_FILTER(1, 3); else HHSR_PNG_FILTER(1, 1);
    } else {
        if (strided) HHSR_PNG_FILTER(2, 3); else HHSR_PNG_FILTER(2, 1);
    }
#undef HHSR_PNG_FILTER
    hipLaunchKernelGGL(k_png_counts_sum, dim3(16), dim3(256), 0, s, (const uint32_t*)scratch, (unsigned)g.filter_groups, counts);
    HHSR_LAUNCHED();
}

// ---- deflate: one dynamic-Huffman block per interval --------------------------------------------------------------------------------
constexpr int PD_CHUNK = 1024;        // stream bytes per pass of a wave: 16 per lane
constexpr int PD_BITS_WORDS = 512;    // 31 carried bits + 1024 x 15 + the end code + 3 = 15409 bits; the header alone: 3700
constexpr unsigned PD_MAX_GRID = 1u << 20;  // waves of a launch; intervals beyond that are walked by stride
static_assert(31 + PD_CHUNK * png::MAX_LEN + png::MAX_LEN + 3 <= (PD_BITS_WORDS - 1) * 32 && png::HDR_MAX_BITS <= (PD_BITS_WORDS - 1) * 32,
              "the bit buffer holds a pass");

// dword `off / 4` of the stream (off a multiple of 4); the bytes at and behind n read as 0 and are never loaded
__device__ __forceinline__ uint32_t png_load_word(const uint8_t* __restrict__ p, size_t off, size_t n) {
    if (off + 4 <= n) return *reinterpret_cast<const uint32_t*>(p + off);
    uint32_t w = 0;
    for (int b = 0; b < 4; ++b)
        if (off + b < n) w |= (uint32_t)p[off + b] << (8 * b);
    return w;
}

__global__ void __launch_bounds__(64) k_png_size(const uint8_t* __restrict__ filtered, size_t N, uint32_t interval, size_t n_int,
                                                  uint32_t* __restrict__ sizes, uint32_t* __restrict__ adler1,
                                                  uint32_t* __restrict__ adler2, png::Codes codes) {
    __shared__ uint8_t lens[png::N_SYM];
    const int lane = threadIdx.x;
    for (int i = lane; i < png::N_SYM; i += 64) lens[i] = (uint8_t)(reinterpret_cast<const uint32_t*>(&codes)[i] >> 16);
    __syncthreads();
    for (size_t it = blockIdx.x; it < n_int; it += gridDim.x) {
        const size_t start = it * interval, end = min(start + interval, N);
        uint64_t nbits = 0, s1 = 0, s2 = 0;  // s2 = sum (end - index) x byte <= 2^20 x 2^20 x 255 / 64 per lane
        for (size_t off = (start & ~(size_t)3) + 4 * (size_t)lane; off < end; off += 256) {
            const uint32_t w = png_load_word(filtered, off, N);
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const size_t idx = off + b;
                if (idx >= start && idx < end) {
                    const uint32_t d = w >> (8 * b) & 255u;
                    nbits += lens[d];
                    s1 += d;
                    s2 += (uint64_t)(end - idx) * d;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            nbits += __shfl_down(nbits, o, 64);
            s1 += __shfl_down(s1, o, 64);
            s2 += __shfl_down(s2, o, 64);
        }
        if (lane == 0) {
            const bool last = it + 1 == n_int;
            const uint64_t total = codes.hdr_bits + nbits + lens[256] + (last ? 0 : 3);
            sizes[it] = (uint32_t)((total + 7) / 8 + (last ? 0 : 4));  // <= (3700 + 2^20 x 15 + 18) / 8 + 5
            adler1[it] = (uint32_t)(s1 % png::ADLER_MOD);
            adler2[it] = (uint32_t)(s2 % png::ADLER_MOD);
        }
    }
}

__global__ void __launch_bounds__(64) k_png_write(const uint8_t* __restrict__ filtered, size_t N, uint32_t interval, size_t n_int,
                                                   const uint64_t* __restrict__ offsets, uint8_t* __restrict__ out,
                                                   size_t capacity, uint32_t* __restrict__ crcs, uint64_t* __restrict__ result,
                                                   png::Codes codes) {
    __shared__ uint32_t code[png::N_SYM];
    __shared__ uint32_t bits[PD_BITS_WORDS];
    __shared__ uint32_t inw[PD_CHUNK / 4 + 2];
    __shared__ uint32_t stride[4][256];
    const int lane = threadIdx.x;
    for (int i = lane; i < png::N_SYM; i += 64) code[i] = reinterpret_cast<const uint32_t*>(&codes)[i];
    for (int i = lane; i < 1024; i += 64) (&stride[0][0])[i] = (&d_crc_stride.t[0][0])[i];
    bool missing = false;  // a byte value without a code
    for (size_t it = blockIdx.x; it < n_int; it += gridDim.x) {
        const size_t start = it * interval, end = min(start + interval, N);
        const bool last = it + 1 == n_int;
        const uint64_t pos = offsets[it];
        const bool word_stores = ((uintptr_t)(out + pos) & 3) == 0;  // (uniform)
        __syncthreads();
        for (int i = lane; i < PD_BITS_WORDS; i += 64) bits[i] = i < png::HDR_WORDS ? codes.hdr[i] | (i == 0 && last ? 1u : 0u) : 0u;
        __syncthreads();
        uint32_t wdone = 0;   // words of the interval that are stored
        uint32_t u = 0;       // the remainder of this lane's words so far is u x^32
        int64_t own_last = -1;  // the last word this lane owned
        // words [0, nwords) of the buffer -> the interval's words wdone ...: stored, and taken into the owner lane's remainder
        auto flush = [&](uint32_t nwords) {
            for (uint32_t i0 = 0; i0 < nwords; i0 += 64) {
                const uint32_t i = i0 + ((uint32_t)(lane - (int)wdone) & 63u);  // (wdone + i) % 64 == lane
                if (i < nwords) {
                    const uint32_t w = bits[i];
                    const uint32_t wi = wdone + i;
                    u = stride[0][u & 255u] ^ stride[1][u >> 8 & 255u] ^ stride[2][u >> 16 & 255u] ^ stride[3][u >> 24] ^ w;
                    own_last = wi;
                    const uint64_t at = pos + 4ull * wi;
                    if (word_stores && at + 4 <= capacity) {
                        *reinterpret_cast<uint32_t*>(out + at) = w;
                    } else {
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if (at + b < capacity) out[at + b] = (uint8_t)(w >> (8 * b));
                    }
                }
            }
            wdone += nwords;
        };
        // after a flush of nwords words: the unfinished word moves to the front of a zeroed buffer
        auto carry_over = [&](uint32_t nwords, uint32_t total) {
            const uint32_t carried = bits[nwords];
            __syncthreads();
            for (uint32_t i = lane; i <= (total >> 5); i += 64) bits[i] = 0;
            __syncthreads();
            if (lane == 0) bits[0] = carried;
            __syncthreads();
        };
        uint32_t carry = codes.hdr_bits;  // bits in the buffer
        flush(carry >> 5);
        carry_over(carry >> 5, carry);
        carry &= 31u;
        uint32_t total = carry;
        for (size_t c0 = start; c0 < end; c0 += PD_CHUNK) {
            const int n = (int)min((size_t)PD_CHUNK, end - c0);
            const size_t a0 = c0 & ~(size_t)3;
            const int sh = (int)(c0 - a0);
            for (int d = lane; d < (sh + n + 3) >> 2; d += 64) inw[d] = png_load_word(filtered, a0 + 4 * (size_t)d, N);
            __syncthreads();
            const int mine = max(0, min(16, n - 16 * lane));
            const uint8_t* my = reinterpret_cast<const uint8_t*>(inw) + sh + 16 * lane;
            uint32_t e[16];
            int len = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                e[j] = j < mine ? code[my[j]] : 0u;
                if (j < mine) missing |= (e[j] >> 16) == 0;
                len += (int)(e[j] >> 16);
            }
            int incl = len;  // inclusive wave prefix sum
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            total = carry + (uint32_t)__shfl(incl, 63, 64);
            {
                const uint32_t p0 = carry + (uint32_t)(incl - len);
                uint32_t wpos = p0 >> 5;
                int nacc = (int)(p0 & 31u);
                uint64_t acc = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    acc |= (uint64_t)(e[j] & 0xffffu) << nacc;  // nacc < 32, a code has at most 15 bits
                    nacc += (int)(e[j] >> 16);
                    if (nacc >= 32) {
                        atomicOr(&bits[wpos], (uint32_t)acc);
                        ++wpos;
                        acc >>= 32;
                        nacc -= 32;
                    }
                }
                if (nacc > 0) atomicOr(&bits[wpos], (uint32_t)acc);
            }
            const bool final_pass = c0 + PD_CHUNK >= end;
            if (final_pass) {  // the end code; in front of the empty stored block its three header bits 000
                if (lane == 0) {
                    const uint64_t v = (uint64_t)(code[256] & 0xffffu) << (total & 31u);
                    atomicOr(&bits[total >> 5], (uint32_t)v);
                    if (v >> 32) atomicOr(&bits[(total >> 5) + 1], (uint32_t)(v >> 32));
                }
                total += (code[256] >> 16) + (last ? 0u : 3u);
                total = (total + 7u) & ~7u;  // zero bits to the byte boundary
            }
            __syncthreads();
            flush(total >> 5);
            if (!final_pass) {
                carry_over(total >> 5, total);
                carry = total & 31u;
            }
        }
        // the interval's remainder: every lane's, moved behind the last whole word, XORed; then the bytes behind that word
        uint32_t r = own_last >= 0 ? png::crc_mul(u, png::crc_xpow8(4ull * (uint64_t)(wdone - own_last), d_crc_powers.x2n)) : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) r ^= __shfl_xor(r, o, 64);
        if (lane == 0) {
            uint64_t at = pos + 4ull * wdone;
            const uint32_t tail = bits[total >> 5];
            for (uint32_t b = 0; b < (total & 31u) >> 3; ++b, ++at) {
                const uint32_t byte = tail >> (8 * b) & 255u;
                r = png::crc_byte(r, byte);
                if (at < capacity) out[at] = (uint8_t)byte;
            }
            if (!last) {  // the empty stored block's LEN and NLEN
                for (int b = 0; b < 4; ++b, ++at) {
                    const uint32_t byte = b < 2 ? 0u : 255u;
                    r = png::crc_byte(r, byte);
                    if (at < capacity) out[at] = (uint8_t)byte;
                }
            }
            crcs[it] = r;
        }
    }
    // (every interval that finds one stores the same word, behind the scan of the sizes; k_png_finish then leaves it alone)
    if (__any(missing) && lane == 0) result[0] = UINT64_MAX;
}

// result[1] = CRC-32 of the deflate stream, result[2] = Adler-32 of the filtered stream, from the intervals' records
__global__ void __launch_bounds__(256) k_png_finish(size_t N, uint32_t interval, size_t n_int, const uint64_t* __restrict__ offsets,
                                                     const uint32_t* __restrict__ sizes, const uint32_t* __restrict__ crcs,
                                                     const uint32_t* __restrict__ adler1, const uint32_t* __restrict__ adler2,
                                                     uint64_t* __restrict__ result) {
    __shared__ uint64_t sm[3][4];
    const int t = threadIdx.x;
    const uint64_t total = result[0];
    if (total == UINT64_MAX) {  // (uniform) a byte value without a code: no stream, no checksums
        if (t == 0) result[1] = result[2] = 0;
        return;
    }
    uint64_t x = 0, s1 = 0, s2 = 0;
    for (size_t k = t; k < n_int; k += 256) {
        const size_t end = min((k + 1) * (size_t)interval, N);
        s1 += adler1[k];  // < 2^31 x 2^16
        s2 = (s2 + adler2[k] + (uint64_t)adler1[k] * ((N - end) % png::ADLER_MOD)) % png::ADLER_MOD;
        x ^= png::crc_mul(crcs[k], png::crc_xpow8(total - offsets[k] - sizes[k], d_crc_powers.x2n));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x ^= __shfl_xor(x, o, 64);
        s1 += __shfl_down(s1, o, 64);
        s2 += __shfl_down(s2, o, 64);
    }
    if ((t & 63) == 0) sm[0][t >> 6] = x, sm[1][t >> 6] = s1, sm[2][t >> 6] = s2;
    __syncthreads();
    if (t == 0) {
        x = sm[0][0] ^ sm[0][1] ^ sm[0][2] ^ sm[0][3];
        s1 = (sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3]) % png::ADLER_MOD;
        s2 = (sm[2][0] + sm[2][1] + sm[2][2] + sm[2][3]) % png::ADLER_MOD;
        const uint32_t crc = (uint32_t)x ^ png::crc_mul(0xFFFFFFFFu, png::crc_xpow8(total, d_crc_powers.x2n)) ^ 0xFFFFFFFFu;
        const uint32_t a = (uint32_t)((1 + s1) % png::ADLER_MOD), b = (uint32_t)((N % png::ADLER_MOD + s2) % png::ADLER_MOD);
        result[1] = crc;
        result[2] = (uint64_t)b << 16 | a;
    }
}

extern "C" int hhsr_png_deflate(const uint8_t* filtered, size_t filtered_bytes, int interval_bytes, const uint8_t* spec,
                                void* scratch, size_t scratch_bytes, uint8_t* out, size_t capacity, uint64_t* result,
                                void* stream) {
    HHSR_ARG(filtered != nullptr && spec != nullptr && scratch != nullptr && out != nullptr && result != nullptr);
    HHSR_ARG(filtered_bytes >= 1 && filtered_bytes <= 0x7fffffffull);
    HHSR_ARG(interval_bytes >= 1 && (uint32_t)interval_bytes <= png::MAX_INTERVAL);
    HHSR_ARG(((uintptr_t)filtered & 3) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)result & 7) == 0);
    const size_t N = filtered_bytes, n_int = (N + (size_t)interval_bytes - 1) / (size_t)interval_bytes;
    const size_t n_groups = (n_int + png::SCAN_GROUP - 1) / png::SCAN_GROUP;
    const size_t need = (n_int + n_groups) * sizeof(uint64_t) + 4 * n_int * sizeof(uint32_t);
    HHSR_ARG(scratch_bytes >= need);
    HHSR_ARG(capacity <= SIZE_MAX - (uintptr_t)out);
    HHSR_ARG(png_disjoint(filtered, N, scratch, need) && png_disjoint(filtered, N, out, capacity) &&
             png_disjoint(filtered, N, result, 24) && png_disjoint(scratch, need, out, capacity) &&
             png_disjoint(scratch, need, result, 24) && png_disjoint(out, capacity, result, 24));
    png::Codes codes;
    const bool spec_is_valid = png::codes_from_spec(spec, &codes);
    HHSR_ARG(spec_is_valid);
    uint64_t* offsets = (uint64_t*)scratch;
    uint64_t* totals = offsets + n_int;
    uint32_t* sizes = (uint32_t*)(totals + n_groups);
    uint32_t* crcs = sizes + n_int;
    uint32_t* adler1 = crcs + n_int;
    uint32_t* adler2 = adler1 + n_int;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t interval = (uint32_t)interval_bytes;
    const dim3 wave(64), wg(256), ints((unsigned)(n_int < PD_MAX_GRID ? n_int : PD_MAX_GRID)), groups((unsigned)n_groups);
    hipLaunchKernelGGL(k_png_size, ints, wave, 0, s, filtered, N, interval, n_int, sizes, adler1, adler2, codes);
    hipLaunchKernelGGL(k_jpeg_group_totals, groups, wg, 0, s, (const uint32_t*)sizes, n_int, totals);
    hipLaunchKernelGGL(k_jpeg_scan_groups, dim3(1), wg, 0, s, totals, n_groups, result);
    hipLaunchKernelGGL(k_jpeg_offsets, groups, wg, 0, s, (const uint32_t*)sizes, n_int, (const uint64_t*)totals, offsets);
    hipLaunchKernelGGL(k_png_write, ints, wave, 0, s, filtered, N, interval, n_int, (const uint64_t*)offsets, out, capacity, crcs,
                       result, codes);
    hipLaunchKernelGGL(k_png_finish, dim3(1), wg, 0, s, N, interval, n_int, (const uint64_t*)offsets, (const uint32_t*)sizes,
                       (const uint32_t*)crcs, (const uint32_t*)adler1, (const uint32_t*)adler2, result);
    HHSR_LAUNCHED();
}
