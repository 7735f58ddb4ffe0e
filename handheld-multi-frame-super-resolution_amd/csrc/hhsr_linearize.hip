// DNG "mapping raw values to linear reference values" (include/hhsr.h: "DNG linearization"): sensor counts -> the
// normalised, white-balanced float32 RAW of hhsr_normalize_raw_u16, with the LinearizationTable, the per-column and
// per-row black deltas and the GainMap opcodes of a camera's file applied on the way.  No counterpart in the reference
// (rawpy does none of it on raw_image).  For pixel (y, x) at CFA position k = (y & 1) * 2 + (x & 1), colour c = cfa[k]:
//
//   lin = table ? table[min(count, table_len - 1)] : count                       (then float32)
//   b   = (float32(black[c]) + delta_h[x]) + delta_v[y];  v = (lin - b) / (float32(white) - b)
//   v  *= g, the bilinear value of the map of position k at the pixel's centre   (only where position k has a map)
//   v  *= float32(wb[c] / wb[1])
//
// float32, every operation rounded once, no contraction (build.py); the map's row / column and fraction in float64.
// 2 B in / 4 B out per pixel like k_normalize_u16, and the same shape: a thread converts 8 pixels of one row with one
// 16-byte load and two 16-byte stores, a workgroup 2048 pixels of one row.
//
// What differs is everything that depends on (y, x) alone and not on the count: b, the denominator and g.  The two
// float64 divisions of a map coordinate are ~25 VALU instructions each, against ~15 for the rest of a pixel, so they
// are NOT done per pixel and frame:
//   frames   a workgroup converts up to LIN_FRAMES (8) frames of its row piece.  b, den and g of a thread's 8 pixels are
//            made once, in registers, and a frame then costs k_normalize_u16's body plus the table read and one
//            multiplication.  A call of one frame pays the coordinates in full; read_dng_burst hands over the whole burst.
//   y        is uniform per workgroup: the first wave blends the map's two rows into tv[parity of x][column] in LDS
//            (at most 2 x 64 floats; lane = column, so the write is conflict-free) — one row coordinate per workgroup,
//            and only the horizontal blend per pixel: two ds_read_b32 whose addresses are equal or adjacent in
//            neighbouring lanes (a map column spans W / 16 pixels), i.e. broadcasts, not a banked gather.
//   table    read through the vector cache and L2, NOT staged in LDS: a workgroup reads 4 KiB of counts per frame, so
//            staging even a 1024-entry table (2 KiB) per workgroup would add half of the kernel's traffic again, and a
//            65536-entry one 32 times it; a workgroup that lived long enough to amortise the copy would be a
//            persistent kernel with one workgroup per CU for the large table.  Counts of neighbouring pixels of one
//            colour are close, so a wave's 64 lookups fall into few cache lines.  One path for every length: there is no
//            LDS / global switch.
// Measured (tools/dng_linearize_time.py, profiles/dng_linearize.txt; 12 MP, us per frame, calls of 8 frames | of 1 frame;
// "scene": a smooth picture with 1 % noise, "random": counts uniform over the table):
//   hhsr_normalize_raw_u16                       13.1 | 17.8
//   nothing to apply                             14.7 | 17.6
//   both deltas                                  14.7 | 18.8     (delta_h as two 16-byte loads; as 8 dwords: 21.8 | 38.8)
//   four 13 x 17 maps                            14.7 | 30.3     (the float64 coordinates: free from 8 frames on)
//   table 1024 / 16384 / 65536, scene            17.6 / 21.9 / 31.9  |  21.2 / 24.6 / 32.3
//   table 1024 / 16384 / 65536, random           20.2 / 39.1 / 47.0  |  23.4 / 38.0 / 49.7
//   table 16384 + deltas + maps, scene (random)  22.1 (37.6) | 33.6 (45.8)
// So everything but the table rides on the sibling's traffic, and the table lookup is what costs: 3 - 9 us per frame on
// picture-like counts up to 16384 entries, 19 us at 65536, and 2 - 3 x the sibling on uniform counts, where every lane
// of a wave reads another cache line.  A table of up to 16384 entries held in LDS by a workgroup that converts
// 8 frames (32 KiB read per 96 KiB of frame traffic) is the follow-up this measurement points at; not built here.
// The 12 % of "nothing to apply" over the sibling in calls of 8 is the group of frames: 8 x fewer workgroups, each with
// 8 loads in flight, against one workgroup per frame and row piece.
#include "hhsr_common.h"

#include <math.h>

#define LIN_FRAMES 8
#define LIN_MAX_POINTS 64

struct LinPhase {  // the map of one position of the 2 x 2 cell
    double origin_v, spacing_v, origin_h, spacing_h;
    int points_v, points_h, offset, has;
};

struct LinArgs {
    float black[4], gain[4];  // per position of the 2x2 CFA cell: (row & 1) * 2 + (col & 1)
    float white;
    int pad;
    LinPhase ph[4];
};

// index pair and fraction of position `pos` of `n` along an axis of a map with P points
__device__ __forceinline__ void lin_axis(int pos, int n, double origin, double spacing, int P, int& i0, int& i1, float& f) {
    i0 = i1 = 0;
    f = 0.0f;
    if (P > 1) {
        const double u = (((double)pos + 0.5) / (double)n - origin) / spacing;
        if (u >= (double)(P - 1)) {
            i0 = i1 = P - 1;
        } else if (u > 0.0) {
            const double fl = floor(u);
            i0 = (int)fl;
            i1 = i0 + 1;
            f = (float)(u - fl);
        }
    }
}

// grid (ceil(W / 2048), H, ceil(n_frames / LIN_FRAMES))
__global__ void __launch_bounds__(256) k_linearize_u16(const uint16_t* __restrict__ raw, int n_frames, int H, int W, int stride,
                                                        size_t frame_in, float* __restrict__ out, size_t frame_out,
                                                        const uint16_t* __restrict__ table, int table_last,
                                                        const float* __restrict__ delta_h, const float* __restrict__ delta_v,
                                                        const float* __restrict__ gains, LinArgs A) {
    __shared__ float tv[2][LIN_MAX_POINTS];
    const int t = threadIdx.x, x0 = (blockIdx.x * 256 + t) * 8, y = blockIdx.y;
    const int r = (y & 1) * 2;
    const LinPhase M0 = A.ph[r], M1 = A.ph[r + 1];  // (uniform: the maps of the row's even and odd columns)
    if (t < HHSR_WAVE) {                            // the first wave: the maps' rows around y, blended
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const LinPhase& M = p ? M1 : M0;
            if (M.has) {
                int r0, r1;
                float fv;
                lin_axis(y, H, M.origin_v, M.spacing_v, M.points_v, r0, r1, fv);
                if (t < M.points_h)
                    tv[p][t] = gains[M.offset + r0 * M.points_h + t] * (1.0f - fv) + gains[M.offset + r1 * M.points_h + t] * fv;
            }
        }
    }
    __syncthreads();
    const int npx = W - x0 < 8 ? W - x0 : 8;  // <= 0: no pixel of this thread's in the row
    if (npx <= 0) return;

    const bool vec = npx == 8 && ((stride | W) & 7) == 0;
    float b[8], den[8], g[8], dh[8];
    const float dv = delta_v ? delta_v[y] : 0.0f;
    if (delta_h && vec && ((uintptr_t)delta_h & 15) == 0) {  // (8 dword loads a thread 32 bytes apart cost more than the frame)
        const float4 lo = reinterpret_cast<const float4*>(delta_h + x0)[0], hi = reinterpret_cast<const float4*>(delta_h + x0)[1];
        dh[0] = lo.x, dh[1] = lo.y, dh[2] = lo.z, dh[3] = lo.w, dh[4] = hi.x, dh[5] = hi.y, dh[6] = hi.z, dh[7] = hi.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) dh[k] = delta_h && k < npx ? delta_h[x0 + k] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int p = k & 1;  // x0 is even: even k are CFA column 0
        const LinPhase& M = p ? M1 : M0;
        b[k] = 0.0f, den[k] = 1.0f, g[k] = 1.0f;
        if (k < npx) {
            b[k] = (A.black[r + p] + dh[k]) + dv;
            den[k] = A.white - b[k];
            if (M.has) {
                int c0, c1;
                float fh;
                lin_axis(x0 + k, W, M.origin_h, M.spacing_h, M.points_h, c0, c1, fh);
                g[k] = tv[p][c0] * (1.0f - fh) + tv[p][c1] * fh;
            }
        }
    }
    const float w0 = A.gain[r], w1 = A.gain[r + 1];
    const int n0 = blockIdx.z * LIN_FRAMES, nf = n_frames - n0 < LIN_FRAMES ? n_frames - n0 : LIN_FRAMES;  // (uniform)
    const uint16_t* __restrict__ src = raw + n0 * frame_in + (size_t)y * stride + x0;
    float* __restrict__ dst = out + n0 * frame_out + (size_t)y * W + x0;
    auto value = [&](uint32_t count, int k) {  // steps 2 - 4 of the contract for pixel k of the thread
        float v = ((float)count - b[k]) / den[k];
        if ((k & 1) ? M1.has : M0.has) v = v * g[k];
        return v * ((k & 1) ? w1 : w0);
    };
    if (vec) {
        // The frames of the group in three passes, each over all of them, so that their loads — and then their table
        // reads — are in flight together: one frame at a time (load, look up, divide, store, next) ran at 1.48 x the
        // sibling's time with nothing to apply.  The counts stay packed two to a register across the passes.
        uint4 q[LIN_FRAMES];
#pragma unroll
        for (int i = 0; i < LIN_FRAMES; ++i)
            if (i < nf) q[i] = *reinterpret_cast<const uint4*>(src + i * frame_in);
        if (table) {
#pragma unroll
            for (int i = 0; i < LIN_FRAMES; ++i) {
                if (i < nf) {
                    uint32_t w[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t lo = table[min(w[k] & 0xffffu, (uint32_t)table_last)];
                        const uint32_t hi = table[min(w[k] >> 16, (uint32_t)table_last)];
                        w[k] = lo | (hi << 16);
                    }
                    q[i] = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < LIN_FRAMES; ++i) {
            if (i < nf) {
                const uint32_t w[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
                float v[8];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[2 * k] = value(w[k] & 0xffffu, 2 * k), v[2 * k + 1] = value(w[k] >> 16, 2 * k + 1);
                float4* o = reinterpret_cast<float4*>(dst + i * frame_out);
                o[0] = make_float4(v[0], v[1], v[2], v[3]);
                o[1] = make_float4(v[4], v[5], v[6], v[7]);
            }
        }
    } else {  // a row's tail, or rows that do not start on 16 bytes: count by count, the same operations
        for (int i = 0; i < nf; ++i) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < npx) {
                    uint32_t c = src[i * frame_in + k];
                    if (table) c = table[min(c, (uint32_t)table_last)];
                    dst[i * frame_out + k] = value(c, k);
                }
            }
        }
    }
}

extern "C" int hhsr_linearize_raw_u16(const uint16_t* raw, int n_frames, int H, int W, int row_stride, const uint8_t cfa[4],
                                      const double* black_levels, double white_level, const double* white_balance,
                                      const uint16_t* table, int table_len, const float* delta_h, const float* delta_v,
                                      const hhsr_gain_map* maps, int n_maps, const float* gains, int64_t gains_len,
                                      float* out, void* stream) {
    HHSR_ARG(raw && cfa && black_levels && white_balance && out);
    HHSR_ARG(n_frames > 0 && H > 0 && W > 0 && row_stride >= W && n_frames <= 65535 && H <= 65535);
    HHSR_ARG(W <= INT32_MAX - 2048);  // the 32-bit pixel indices of a row's last workgroup
    HHSR_ARG(((uintptr_t)raw & 15) == 0 && ((uintptr_t)out & 15) == 0);
    HHSR_ARG(white_balance[1] != 0.0);
    HHSR_ARG(table == nullptr ? table_len == 0 : (table_len >= 1 && table_len <= 65536));
    HHSR_ARG(((uintptr_t)table & 1) == 0 && ((uintptr_t)delta_h & 3) == 0 && ((uintptr_t)delta_v & 3) == 0);
    HHSR_ARG(n_maps >= 0 && n_maps <= HHSR_MAX_GAIN_MAPS);
    HHSR_ARG(n_maps == 0 || (maps != nullptr && gains != nullptr && ((uintptr_t)gains & 3) == 0));
    HHSR_ARG(n_maps == 0 || (gains_len >= 1 && gains_len <= INT32_MAX));
    LinArgs A;
    A.pad = 0;
    A.white = (float)white_level;
    for (int k = 0; k < 4; ++k) {
        HHSR_ARG(cfa[k] <= 2);
        const int c = cfa[k];
        A.black[k] = (float)black_levels[c];
        A.gain[k] = (float)(white_balance[c] / white_balance[1]);  // the cast of hhsr_normalize_raw_u16
        A.ph[k] = LinPhase{0.0, 1.0, 0.0, 1.0, 1, 1, 0, 0};
    }
    for (int i = 0; i < n_maps; ++i) {
        const hhsr_gain_map& m = maps[i];
        HHSR_ARG(m.points_v >= 1 && m.points_v <= LIN_MAX_POINTS && m.points_h >= 1 && m.points_h <= LIN_MAX_POINTS);
        HHSR_ARG(m.offset >= 0 && m.offset <= gains_len - (int64_t)m.points_v * m.points_h);
        HHSR_ARG(isfinite(m.origin_v) && isfinite(m.origin_h));
        HHSR_ARG(m.points_v == 1 || (isfinite(m.spacing_v) && m.spacing_v > 0.0));
        HHSR_ARG(m.points_h == 1 || (isfinite(m.spacing_h) && m.spacing_h > 0.0));
        const bool all = m.row_pitch == 1 && m.col_pitch == 1;
        HHSR_ARG(all || (m.row_pitch == 2 && m.col_pitch == 2));
        HHSR_ARG(all ? (m.top == 0 && m.left == 0 && n_maps == 1) : ((m.top | m.left) >= 0 && m.top <= 1 && m.left <= 1));
        const LinPhase P = {m.origin_v, m.spacing_v, m.origin_h, m.spacing_h, m.points_v, m.points_h, (int)m.offset, 1};
        for (int k = 0; k < 4; ++k) {
            if (all || k == m.top * 2 + m.left) {
                HHSR_ARG(!A.ph[k].has);  // at most one map per position of the cell
                A.ph[k] = P;
            }
        }
    }
    const dim3 grid(hhsr_cdiv(hhsr_cdiv(W, 8), 256), H, hhsr_cdiv(n_frames, LIN_FRAMES));
    hipLaunchKernelGGL(k_linearize_u16, grid, dim3(256), 0, (hipStream_t)stream, raw, n_frames, H, W, row_stride,
                       (size_t)H * row_stride, out, (size_t)H * W, table, table_len - 1, delta_h, delta_v, gains, A);
    HHSR_LAUNCHED();
}
