// DNG output: the image's uint16 samples -> lossless-JPEG tile streams, coded on the device (include/hhsr.h, "DNG output:
// lossless JPEG").  The per-sample rule, Annex K.2, the stream's fixed bytes and the host encoder live in
// hhsr_ljpeg_enc_core.h; this unit holds the C ABI and the kernels.
//
// Unlike its decoder a lossless-JPEG encoder is parallel: every prediction comes from the ORIGINAL samples, so the bits of
// every sample are independent and only their positions need a prefix sum.
//
// k_ljpeg_hist    a workgroup takes batches of LE_BATCH samples (any tile's), every thread LE_PER consecutive ones of a line;
//                 categories are counted with LDS atomics into 32 copies of the [4][17] table (the lanes of a wave spread over
//                 them: three or four categories take nearly all samples), one partial table per workgroup, summed by
//                 k_ljpeg_hist_sum: integers, no atomics on device memory.
// k_ljpeg_tile    one workgroup of 256 threads per tile stream, which starts byte-aligned, so tiles are independent.  It walks
//                 the stream in batches of LE_BATCH samples: a thread loads its LE_PER samples and their neighbours Ra, Rb, Rc
//                 straight from the image (dword loads where the image allows them; the edge replicated sample by sample),
//                 forms code word and magnitude bits, a workgroup prefix sum of the bit lengths places them, and they are
//                 OR-ed into the LDS bit buffer (most significant bit first; OR commutes, so the result does not depend on
//                 the order).  Then the bytes: a thread takes LE_RUN consecutive bytes of the buffer, counts its FF bytes, a
//                 second prefix sum gives the stuffed position, the bytes (FF as FF 00) go into an LDS byte buffer that is
//                 misaligned like the destination, and leave as aligned dwords, every position compared with the capacity.
//                 The unfinished byte of a batch is carried into the next.  WRITE = false is the size pass (the stuffing
//                 depends on the bytes, so the bits are formed twice), around the offsets scan of hhsr_jpeg.hip (hhsr_scan.h).
#include "hhsr_common.h"
#include "hhsr_ljpeg_enc_core.h"
#include "hhsr_jpeg_tables.h"
#include "hhsr_scan.h"

namespace lje = hhsr_lje;

static_assert(lje::SCAN_GROUP == jpeg::SCAN_GROUP, "the offsets scan of hhsr_jpeg.hip works on groups of jpeg::SCAN_GROUP");

namespace {

constexpr int LE_THREADS = 256;
constexpr int LE_PER = 8;  // samples per thread and batch: a line of a tile is a multiple of 16 samples, so a run never leaves it
constexpr int LE_BATCH = LE_THREADS * LE_PER;
constexpr int LE_BIT_WORDS = 2048;  // 7 carried bits + LE_BATCH x 31 + 7 pad bits
constexpr int LE_MAX_BYTES = (7 + LE_BATCH * lje::MAX_BITS + 7) / 8;  // bytes a batch completes
constexpr int LE_RUN = 32;          // bytes per thread of the stuffing step
constexpr int LE_OUT_WORDS = (3 + 2 * LE_MAX_BYTES + 3) / 4 + 1;
constexpr unsigned LE_MAX_GRID = 2048;  // workgroups of a launch, two rounds of what the chip holds; tiles beyond are walked by stride
constexpr int LE_HIST_COPIES = 32;
constexpr int LE_HIST_STRIDE = lje::HIST_STRIDE;
static_assert(7 + LE_BATCH * lje::MAX_BITS + 7 <= (LE_BIT_WORDS - 1) * 32, "the bit buffer holds a batch");
static_assert(LE_THREADS * LE_RUN >= LE_MAX_BYTES, "the stuffing step covers a batch");
static_assert(LE_HIST_STRIDE > HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT, "a partial table holds the counts and the flag");

struct LeArgs {
    const uint16_t* img;
    int H, W;
    int64_t row_elems;
    int P, predictor, tile_h, tile_w, tiles_x;
    uint32_t tile_samples, batches;  // per tile
    uint64_t n_tiles;
    bool vec;  // img 4-byte aligned and row_elems even: runs inside the image are loaded as dwords
};

// Elements r0 - 4 .. r0 + 7 of line `iy` of the image as tile (.., x0) sees it (element r of a tile's line: pixel r / NF,
// component r % NF; pixels right of the image replicate the last): v[4 + j] for j = -NF .. 7, zero where r0 + j < 0.
template <int NF>
__device__ __forceinline__ void le_load_run(const LeArgs& a, int iy, int x0, int r0, int32_t* v) {
    const uint16_t* __restrict__ row = a.img + (int64_t)iy * a.row_elems;
    if (a.vec && r0 >= 8 && x0 + (r0 + LE_PER - 1) / NF < a.W) {  // (r0 is a multiple of 8, x0 NF even: the dwords are aligned)
        const uint32_t* w = reinterpret_cast<const uint32_t*>(row + (int64_t)x0 * NF + r0 - 4);
#pragma unroll
        for (int k = (NF > 2 ? 0 : 1); k < 6; ++k) {
            const uint32_t d = w[k];
            v[2 * k] = (int32_t)(d & 0xFFFFu);
            v[2 * k + 1] = (int32_t)(d >> 16);
        }
        return;
    }
#pragma unroll
    for (int j = -NF; j < LE_PER; ++j) {
        const int r = r0 + j;
        int32_t s = 0;
        if (r >= 0) {
            const int x = min(x0 + r / NF, a.W - 1);
            s = row[(int64_t)x * NF + r % NF];
        }
        v[4 + j] = s;
    }
}

// The LE_PER samples from element idx of tile (y0, x0) on, and their predictions.
template <int NF>
__device__ __forceinline__ void le_run(const LeArgs& a, int y0, int x0, uint32_t idx, int32_t* s, int32_t* p, int* c0) {
    const uint32_t line = (uint32_t)a.tile_w * NF;
    const int y = (int)(idx / line), r0 = (int)(idx % line);
    int32_t cur[4 + LE_PER], up[4 + LE_PER];
    le_load_run<NF>(a, min(y0 + y, a.H - 1), x0, r0, cur);
    const bool need_up = y > 0 && (a.predictor != 1 || r0 == 0);
    if (need_up) {
        le_load_run<NF>(a, min(y0 + y - 1, a.H - 1), x0, r0, up);
    } else {
#pragma unroll
        for (int j = 0; j < 4 + LE_PER; ++j) up[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < LE_PER; ++j) {
        const int x = (r0 + j) / NF;
        s[j] = cur[4 + j];
        p[j] = lje::predict(a.predictor, a.P, y, x, cur[4 + j - NF], up[4 + j], up[4 + j - NF]);
    }
    *c0 = r0 % NF;
}

// exclusive prefix sum of v over the workgroup, and the total; two barriers (the first guards `wsum` against its last readers)
__device__ __forceinline__ uint32_t le_block_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < LE_THREADS / 64; ++w) {
        const uint32_t x = wsum[w];
        base += w < wave ? x : 0u;
        tot += x;
    }
    *total = tot;
    return base + incl - v;
}

template <int NF>
__global__ void __launch_bounds__(LE_THREADS) k_ljpeg_hist(LeArgs a, uint64_t* __restrict__ partial) {
    __shared__ uint32_t cnt[LE_HIST_COPIES][HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT];
    __shared__ uint32_t bad_s;
    const int t = threadIdx.x;
    for (int i = t; i < LE_HIST_COPIES * HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT; i += LE_THREADS) (&cnt[0][0])[i] = 0;
    if (t == 0) bad_s = 0;
    __syncthreads();
    uint32_t* mine = cnt[t & (LE_HIST_COPIES - 1)];
    bool bad = false;
    const uint64_t items = a.n_tiles * a.batches;
    for (uint64_t it = blockIdx.x; it < items; it += gridDim.x) {  // (a workgroup counts at most 2^30 samples: geom())
        const uint64_t tile = it / a.batches;
        const uint32_t idx = (uint32_t)(it % a.batches) * LE_BATCH + (uint32_t)t * LE_PER;
        if (idx >= a.tile_samples) continue;
        const int y0 = (int)(tile / a.tiles_x) * a.tile_h, x0 = (int)(tile % a.tiles_x) * a.tile_w;
        int32_t s[LE_PER], p[LE_PER];
        int c;
        le_run<NF>(a, y0, x0, idx, s, p, &c);
#pragma unroll
        for (int j = 0; j < LE_PER; ++j) {
            int32_t d;
            const int ssss = lje::category(s[j], p[j], &d);
            bad |= (s[j] >> a.P) != 0;
            atomicAdd(&mine[c * lje::N_CAT + ssss], 1u);
            c = c + 1 == NF ? 0 : c + 1;
        }
    }
    if (bad) bad_s = 1;  // (every writer stores the same value)
    __syncthreads();
    uint64_t* out = partial + (size_t)blockIdx.x * LE_HIST_STRIDE;
    if (t < HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT) {
        uint64_t sum = 0;
        for (int k = 0; k < LE_HIST_COPIES; ++k) sum += cnt[k][t];
        out[t] = sum;
    } else if (t == HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT) {
        out[t] = bad_s;
    }
}

__global__ void __launch_bounds__(128) k_ljpeg_hist_sum(const uint64_t* __restrict__ partial, unsigned n_partial, int Nf,
                                                        uint64_t* __restrict__ counts, uint32_t* __restrict__ status) {
    const int t = threadIdx.x;
    if (t > HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT) return;
    uint64_t sum = 0;
    for (unsigned g = 0; g < n_partial; ++g) sum += partial[(size_t)g * LE_HIST_STRIDE + t];
    if (t == HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT) *status = sum ? HHSR_LJPEG_BAD_SAMPLE : HHSR_LJPEG_OK;
    else if (t < Nf * lje::N_CAT) counts[t] = sum;
}

// byte k of the bit buffer (bit 0 of the stream is bit 31 of word 0)
__device__ __forceinline__ uint32_t le_byte(uint32_t w, int b) { return w >> (24 - 8 * b) & 255u; }

template <int NF, bool WRITE>
__global__ void __launch_bounds__(LE_THREADS) k_ljpeg_tile(LeArgs a, uint32_t* __restrict__ sizes, uint32_t* __restrict__ tile_bytes,
                                                           uint64_t* __restrict__ offsets, uint8_t* __restrict__ out, uint64_t capacity,
                                                           uint64_t* __restrict__ length, lje::Codes codes) {
    __shared__ uint32_t code[HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT];
    __shared__ __attribute__((aligned(16))) uint32_t bits[LE_BIT_WORDS];
    __shared__ __attribute__((aligned(16))) uint32_t sout[WRITE ? LE_OUT_WORDS : 1];
    __shared__ uint32_t wsum[LE_THREADS / 64];
    const int t = threadIdx.x;
    if (t < HHSR_LJPEG_MAX_COMPONENTS * lje::N_CAT) code[t] = (&codes.e[0][0])[t];
    bool bad = false;  // a category without a code, a sample at or above 2^P
    for (uint64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int y0 = (int)(tile / a.tiles_x) * a.tile_h, x0 = (int)(tile % a.tiles_x) * a.tile_w;
        const uint64_t pos = WRITE ? offsets[tile] : 0;
        if (WRITE && t < (int)codes.header_bytes && pos + t < capacity) out[pos + t] = codes.header[t];
        uint64_t gpos = pos + codes.header_bytes;  // where the next byte of the scan goes
        uint32_t carry = 0, carried = 0;           // bits of the unfinished byte, and the byte (its low bits 0)
        uint32_t used = LE_BIT_WORDS;              // words of the buffer that may be set
        for (uint32_t b = 0; b < a.batches; ++b) {
            __syncthreads();  // the buffer's last readers are done
            for (uint32_t i = t; i < used; i += LE_THREADS) bits[i] = i == 0 ? carried << 24 : 0u;
            const uint32_t idx = b * LE_BATCH + (uint32_t)t * LE_PER;
            uint32_t val[LE_PER], len[LE_PER], mylen = 0;
            if (idx < a.tile_samples) {
                int32_t s[LE_PER], p[LE_PER];
                int c;
                le_run<NF>(a, y0, x0, idx, s, p, &c);
#pragma unroll
                for (int j = 0; j < LE_PER; ++j) {
                    lje::sample_bits(s[j], p[j], code + c * lje::N_CAT, &val[j], &len[j]);
                    bad |= len[j] == 0 || (s[j] >> a.P) != 0;
                    mylen += len[j];
                    c = c + 1 == NF ? 0 : c + 1;
                }
            } else {
#pragma unroll
                for (int j = 0; j < LE_PER; ++j) val[j] = len[j] = 0;
            }
            uint32_t total;
            const uint32_t at = carry + le_block_scan(mylen, wsum, &total);  // (its barriers: the buffer is zeroed)
            {
                uint32_t wpos = at >> 5;
                int n = (int)(at & 31u);  // bits of word wpos in front of this thread's
                uint64_t acc = 0;
#pragma unroll
                for (int j = 0; j < LE_PER; ++j) {
                    acc = (acc << len[j]) | val[j];  // n < 32, a sample has at most 31 bits
                    n += (int)len[j];
                    if (n >= 32) {
                        atomicOr(&bits[wpos], (uint32_t)(acc >> (n - 32)));
                        ++wpos;
                        n -= 32;
                        acc &= (1ull << n) - 1ull;
                    }
                }
                if (n > 0 && mylen > 0) atomicOr(&bits[wpos], (uint32_t)(acc << (32 - n)));
            }
            total += carry;
            if (b + 1 == a.batches) {  // 1-bits up to the byte boundary: inside the byte, so inside the word
                const uint32_t pad = (8u - (total & 7u)) & 7u;
                if (t == 0 && pad) atomicOr(&bits[total >> 5], ((1u << pad) - 1u) << (32u - (total & 31u) - pad));
                total += pad;
            }
            __syncthreads();
            const uint32_t nb = total >> 3;  // whole bytes
            const uint32_t k0 = (uint32_t)t * LE_RUN;
            uint32_t w[LE_RUN / 4], ff = 0;
            if (k0 < nb) {
#pragma unroll
                for (int i = 0; i < LE_RUN / 4; ++i) {
                    w[i] = bits[k0 / 4 + i];
#pragma unroll
                    for (int q = 0; q < 4; ++q) ff += (k0 + 4 * i + q < nb && le_byte(w[i], q) == 255u) ? 1u : 0u;
                }
            }
            uint32_t ff_total;
            const uint32_t ff_before = le_block_scan(ff, wsum, &ff_total);
            const uint32_t nbs = nb + ff_total;  // stuffed bytes of this batch
            if (WRITE) {
                const uint32_t mis = (uint32_t)((uintptr_t)(out + gpos) & 3u);  // sout[i] is byte gpos - mis + i of out
                uint8_t* so = reinterpret_cast<uint8_t*>(sout);
                if (k0 < nb) {
                    uint32_t d = mis + k0 + ff_before;
#pragma unroll
                    for (int i = 0; i < LE_RUN / 4; ++i) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if (k0 + 4 * i + q < nb) {
                                const uint32_t v = le_byte(w[i], q);
                                so[d++] = (uint8_t)v;
                                if (v == 255u) so[d++] = 0;
                            }
                        }
                    }
                }
                __syncthreads();
                const uint32_t end = mis + nbs;
                const uint64_t g0 = gpos - mis;
                for (uint32_t i0 = 4 * (uint32_t)t; i0 < end; i0 += 4 * LE_THREADS) {
                    if (i0 >= mis && i0 + 4 <= end && g0 + i0 + 4 <= capacity) {
                        *reinterpret_cast<uint32_t*>(out + g0 + i0) = sout[i0 >> 2];
                    } else {
                        for (uint32_t i = max(i0, mis); i < min(i0 + 4, end); ++i)
                            if (g0 + i < capacity) out[g0 + i] = so[i];
                    }
                }
            }
            carry = total & 7u;
            carried = carry ? le_byte(bits[nb >> 2], (int)(nb & 3u)) : 0u;
            used = (total >> 5) + 1;
            gpos += nbs;
        }
        if (t == 0) {
            const uint64_t len = gpos + 2 - pos;  // with EOI
            if (WRITE) {
                if (gpos < capacity) out[gpos] = 0xFF;
                if (gpos + 1 < capacity) out[gpos + 1] = 0xD9;
                if ((len & 1) && gpos + 2 < capacity) out[gpos + 2] = 0;  // the next stream starts at an even offset
                if (tile + 1 == a.n_tiles) offsets[a.n_tiles] = pos + len + (len & 1);
            } else {
                sizes[tile] = (uint32_t)(len + (len & 1));
                tile_bytes[tile] = (uint32_t)len;
            }
        }
    }
    // (every workgroup that finds one stores the same word, behind the scan that set the length)
    if (WRITE && __any(bad) && (t & 63) == 0) *length = UINT64_MAX;
}

inline bool le_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}

#define LE_ARG(cond)                                               \
    do {                                                           \
        if (!(cond)) {                                             \
            hhsr_set_error("%s: invalid argument: %s", fn, #cond); \
            return -1;                                             \
        }                                                          \
    } while (0)

// what every entry point that sees the samples checks; *g is set
int le_check_image(const char* fn, const uint16_t* samples, int H, int W, int Nf, int64_t row_elems, int P, int predictor,
                   int tile_h, int tile_w, lje::Geom* g, size_t* image_bytes) {
    LE_ARG(samples != nullptr && ((uintptr_t)samples & 1) == 0);
    LE_ARG(P >= 2 && P <= 16 && predictor >= 1 && predictor <= 7);
    const bool dimensions_and_tile_are_valid = lje::geom(H, W, Nf, tile_h, tile_w, g);
    LE_ARG(dimensions_and_tile_are_valid /* H, W >= 1; Nf 1..4; tile 16..65535, multiples of 16, tile_h tile_w Nf <= 2^28 */);
    LE_ARG(row_elems >= (int64_t)W * Nf && row_elems <= ((int64_t)1 << 40));
    *image_bytes = (size_t)(((int64_t)(H - 1) * row_elems + (int64_t)W * Nf) * 2);
    return 0;
}

LeArgs le_args(const uint16_t* samples, int H, int W, int Nf, int64_t row_elems, int P, int predictor, int tile_h, int tile_w,
               const lje::Geom& g) {
    LeArgs a{};
    a.img = samples;
    a.H = H, a.W = W, a.row_elems = row_elems;
    a.P = P, a.predictor = predictor, a.tile_h = tile_h, a.tile_w = tile_w, a.tiles_x = g.tiles_x;
    a.tile_samples = (uint32_t)g.tile_samples;
    a.batches = (uint32_t)((g.tile_samples + LE_BATCH - 1) / LE_BATCH);
    a.n_tiles = g.n_tiles;
    a.vec = ((uintptr_t)samples & 3) == 0 && (row_elems & 1) == 0;
    return a;
}

int le_check_encode(const char* fn, const uint16_t* samples, size_t image_bytes, const lje::Geom& g, const uint8_t* bits,
                    const uint8_t* values, uint8_t* out, size_t capacity, uint64_t* offsets, uint32_t* tile_bytes,
                    uint64_t* length) {
    LE_ARG(bits != nullptr && values != nullptr && out != nullptr && offsets != nullptr && tile_bytes != nullptr && length != nullptr);
    LE_ARG(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)tile_bytes & 3) == 0 && ((uintptr_t)length & 7) == 0);
    LE_ARG(capacity <= SIZE_MAX - (uintptr_t)out);
    const size_t no = (g.n_tiles + 1) * 8, nt = g.n_tiles * 4;
    LE_ARG(le_disjoint(samples, image_bytes, out, capacity) && le_disjoint(samples, image_bytes, offsets, no) &&
           le_disjoint(samples, image_bytes, tile_bytes, nt) && le_disjoint(samples, image_bytes, length, 8) &&
           le_disjoint(out, capacity, offsets, no) && le_disjoint(out, capacity, tile_bytes, nt) &&
           le_disjoint(out, capacity, length, 8) && le_disjoint(offsets, no, tile_bytes, nt) &&
           le_disjoint(offsets, no, length, 8) && le_disjoint(tile_bytes, nt, length, 8));
    return 0;
}

}  // namespace

extern "C" int hhsr_ljpeg_encode_workspace(int H, int W, int Nf, int tile_h, int tile_w, size_t* scratch_bytes, size_t* max_bytes) {
    HHSR_ARG(scratch_bytes != nullptr && max_bytes != nullptr);
    lje::Geom g;
    const bool dimensions_and_tile_are_valid = lje::geom(H, W, Nf, tile_h, tile_w, &g);
    HHSR_ARG(dimensions_and_tile_are_valid /* H, W >= 1; Nf 1..4; tile 16..65535, multiples of 16, tile_h tile_w Nf <= 2^28 */);
    *scratch_bytes = (size_t)g.scratch_bytes;
    *max_bytes = (size_t)g.max_bytes;
    return 0;
}

extern "C" int hhsr_ljpeg_huffman(const uint64_t* counts, uint8_t* bits, uint8_t* values, int* n_values) {
    HHSR_ARG(counts != nullptr && bits != nullptr && values != nullptr && n_values != nullptr);
    HHSR_ARG(((uintptr_t)counts & 7) == 0);
    uint8_t b[16], v[17];
    int n = 0;
    const bool counts_are_usable = lje::build_k2(counts, b, v, &n);
    HHSR_ARG(counts_are_usable /* one of the 17 is set, the sum is at most 2^62 */);
    for (int i = 0; i < 16; ++i) bits[i] = b[i];
    for (int i = 0; i < 17; ++i) values[i] = v[i];
    *n_values = n;
    return 0;
}

extern "C" int hhsr_ljpeg_histogram(const uint16_t* samples, int H, int W, int Nf, int64_t row_elems, int P, int predictor,
                                    int tile_h, int tile_w, uint64_t* counts, uint32_t* status, void* scratch,
                                    size_t scratch_bytes, void* stream) {
    const char* fn = __func__;
    lje::Geom g;
    size_t image_bytes;
    if (int rc = le_check_image(fn, samples, H, W, Nf, row_elems, P, predictor, tile_h, tile_w, &g, &image_bytes)) return rc;
    LE_ARG(counts != nullptr && status != nullptr && scratch != nullptr);
    LE_ARG(((uintptr_t)counts & 7) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)scratch & 7) == 0);
    LE_ARG(scratch_bytes >= g.scratch_bytes);
    const size_t nc = (size_t)Nf * lje::N_CAT * 8;
    LE_ARG(le_disjoint(samples, image_bytes, counts, nc) && le_disjoint(samples, image_bytes, status, 4) &&
           le_disjoint(samples, image_bytes, scratch, g.scratch_bytes) && le_disjoint(counts, nc, status, 4) &&
           le_disjoint(counts, nc, scratch, g.scratch_bytes) && le_disjoint(status, 4, scratch, g.scratch_bytes));
    const LeArgs a = le_args(samples, H, W, Nf, row_elems, P, predictor, tile_h, tile_w, g);
    const uint64_t items = a.n_tiles * a.batches;
    const unsigned groups = (unsigned)(items < (uint64_t)lje::HIST_MAX_GROUPS ? items : (uint64_t)lje::HIST_MAX_GROUPS);
    hipStream_t s = (hipStream_t)stream;
    uint64_t* partial = (uint64_t*)scratch;
    switch (Nf) {
        case 1: hipLaunchKernelGGL(k_ljpeg_hist<1>, dim3(groups), dim3(LE_THREADS), 0, s, a, partial); break;
        case 2: hipLaunchKernelGGL(k_ljpeg_hist<2>, dim3(groups), dim3(LE_THREADS), 0, s, a, partial); break;
        case 3: hipLaunchKernelGGL(k_ljpeg_hist<3>, dim3(groups), dim3(LE_THREADS), 0, s, a, partial); break;
        default: hipLaunchKernelGGL(k_ljpeg_hist<4>, dim3(groups), dim3(LE_THREADS), 0, s, a, partial); break;
    }
    hipLaunchKernelGGL(k_ljpeg_hist_sum, dim3(1), dim3(128), 0, s, (const uint64_t*)partial, groups, Nf, counts, status);
    HHSR_LAUNCHED();
}

extern "C" int hhsr_ljpeg_encode(const uint16_t* samples, int H, int W, int Nf, int64_t row_elems, int P, int predictor,
                                 int tile_h, int tile_w, const uint8_t* bits, const uint8_t* values, void* scratch,
                                 size_t scratch_bytes, uint8_t* out, size_t capacity, uint64_t* offsets, uint32_t* tile_bytes,
                                 uint64_t* length, void* stream) {
    const char* fn = __func__;
    lje::Geom g;
    size_t image_bytes;
    if (int rc = le_check_image(fn, samples, H, W, Nf, row_elems, P, predictor, tile_h, tile_w, &g, &image_bytes)) return rc;
    if (int rc = le_check_encode(fn, samples, image_bytes, g, bits, values, out, capacity, offsets, tile_bytes, length)) return rc;
    LE_ARG(scratch != nullptr && ((uintptr_t)scratch & 7) == 0 && scratch_bytes >= g.scratch_bytes);
    LE_ARG(le_disjoint(scratch, g.scratch_bytes, samples, image_bytes) && le_disjoint(scratch, g.scratch_bytes, out, capacity) &&
           le_disjoint(scratch, g.scratch_bytes, offsets, (g.n_tiles + 1) * 8) &&
           le_disjoint(scratch, g.scratch_bytes, tile_bytes, g.n_tiles * 4) && le_disjoint(scratch, g.scratch_bytes, length, 8));
    lje::Codes codes;
    const bool tables_are_prefix_codes = lje::make_codes(bits, values, Nf, P, predictor, tile_h, tile_w, &codes);
    LE_ARG(tables_are_prefix_codes /* per component 1..17 distinct values <= 16, Kraft sum <= 1 */);
    const LeArgs a = le_args(samples, H, W, Nf, row_elems, P, predictor, tile_h, tile_w, g);
    uint64_t* totals = (uint64_t*)scratch;
    uint32_t* sizes = (uint32_t*)(totals + g.n_groups);
    hipStream_t s = (hipStream_t)stream;
    const dim3 tiles((unsigned)(g.n_tiles < LE_MAX_GRID ? g.n_tiles : LE_MAX_GRID)), wg(LE_THREADS), groups((unsigned)g.n_groups);
#define LE_LAUNCH(NF, WRITE)                                                                                                  \
    hipLaunchKernelGGL((k_ljpeg_tile<NF, WRITE>), tiles, wg, 0, s, a, sizes, tile_bytes, offsets, out, (uint64_t)capacity, \
                       length, codes)
#define LE_LAUNCH_NF(WRITE)                    \
    switch (Nf) {                              \
        case 1: LE_LAUNCH(1, WRITE); break;    \
        case 2: LE_LAUNCH(2, WRITE); break;    \
        case 3: LE_LAUNCH(3, WRITE); break;    \
        default: LE_LAUNCH(4, WRITE); break;   \
    }
    LE_LAUNCH_NF(false);
    hipLaunchKernelGGL(k_jpeg_group_totals, groups, wg, 0, s, (const uint32_t*)sizes, (size_t)g.n_tiles, totals);
    hipLaunchKernelGGL(k_jpeg_scan_groups, dim3(1), wg, 0, s, totals, (size_t)g.n_groups, length);
    hipLaunchKernelGGL(k_jpeg_offsets, groups, wg, 0, s, (const uint32_t*)sizes, (size_t)g.n_tiles, (const uint64_t*)totals, offsets);
    LE_LAUNCH_NF(true);
#undef LE_LAUNCH_NF
#undef LE_LAUNCH
    HHSR_LAUNCHED();
}

extern "C" int hhsr_ljpeg_encode_host(const uint16_t* samples, int H, int W, int Nf, int64_t row_elems, int P, int predictor,
                                      int tile_h, int tile_w, const uint8_t* bits, const uint8_t* values, uint8_t* out,
                                      size_t capacity, uint64_t* offsets, uint32_t* tile_bytes, uint64_t* length) {
    const char* fn = __func__;
    lje::Geom g;
    size_t image_bytes;
    if (int rc = le_check_image(fn, samples, H, W, Nf, row_elems, P, predictor, tile_h, tile_w, &g, &image_bytes)) return rc;
    if (int rc = le_check_encode(fn, samples, image_bytes, g, bits, values, out, capacity, offsets, tile_bytes, length)) return rc;
    lje::Codes codes;
    const bool tables_are_prefix_codes = lje::make_codes(bits, values, Nf, P, predictor, tile_h, tile_w, &codes);
    LE_ARG(tables_are_prefix_codes /* per component 1..17 distinct values <= 16, Kraft sum <= 1 */);
    lje::encode_image(samples, H, W, Nf, row_elems, P, predictor, tile_h, tile_w, codes, g, out, (uint64_t)capacity, offsets,
                      tile_bytes, length);
    return 0;
}
