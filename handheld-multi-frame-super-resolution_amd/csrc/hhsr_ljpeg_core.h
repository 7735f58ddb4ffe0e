// Lossless JPEG (ITU-T T.81 Annex H, SOF3) as DNG Compression 7 holds it: the marker parser, the decode tables and the
// decoder of ONE stream, in plain C++ that compiles for the host alone (no HIP header when __HIPCC__ is undefined:
// tests/ljpeg_fuzz_main.cpp builds it with clang++ under sanitizers) and, inside hhsr_ljpeg.hip, for host and device.
// include/hhsr.h, section "DNG input: lossless JPEG", states the contract; this file is its one implementation.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/hhsr.h"

#if defined(__HIPCC__)
#define HHSR_LJ_HD __host__ __device__ __forceinline__
#else
#define HHSR_LJ_HD inline
#endif

namespace hhsr_lj {

constexpr int64_t MAX_SAMPLES = (int64_t)1 << 28;  // X Y Nf of one stream: the loop count the decoder accepts

// ---- marker segments (host) -------------------------------------------------------------------------------------------
// nullptr, or the reason `s[0 .. n)` is refused; *info is complete only for nullptr.  Every index is checked against n.
inline const char* parse(const uint8_t* s, size_t n, hhsr_ljpeg_info* info) {
    if (!s || !info) return "null pointer";
    *info = hhsr_ljpeg_info{};
    if (n < 4 || s[0] != 0xFF || s[1] != 0xD8) return "no SOI marker";
    size_t p = 2;
    bool have_sof = false;
    for (;;) {
        if (p + 4 > n) return "marker segment behind the end of the stream";
        if (s[p] != 0xFF) return "marker expected";
        const int m = s[p + 1];
        if (m == 0xFF) {  // fill byte
            ++p;
            continue;
        }
        if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) return "unexpected marker before the scan";
        const size_t len = ((size_t)s[p + 2] << 8) | s[p + 3];
        if (len < 2 || p + 2 + len > n) return "marker length outside the stream";
        const uint8_t* b = s + p + 4;  // payload, len - 2 bytes
        const size_t nb = len - 2;
        if (m == 0xC3) {
            if (have_sof) return "second frame header";
            if (nb < 6) return "SOF3 too short";
            info->P = b[0];
            info->Y = (b[1] << 8) | b[2];
            info->X = (b[3] << 8) | b[4];
            info->Nf = b[5];
            if (info->P < 2 || info->P > 16) return "precision P outside 2..16";
            if (info->Nf < 1 || info->Nf > HHSR_LJPEG_MAX_COMPONENTS) return "components Nf outside 1..4";
            if (info->X < 1 || info->Y < 1) return "X or Y is zero (DNL is not supported)";
            if (nb != (size_t)6 + 3 * (size_t)info->Nf) return "SOF3 length does not match Nf";
            for (int c = 0; c < info->Nf; ++c) {
                info->component_id[c] = b[6 + 3 * c];
                if (b[7 + 3 * c] != 0x11) return "sampling factors H, V other than 1";
                for (int d = 0; d < c; ++d)
                    if (info->component_id[d] == info->component_id[c]) return "duplicate component id";
            }
            have_sof = true;
        } else if ((m >= 0xC0 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return "SOF other than SOF3 (lossless, Huffman)";
        } else if (m == 0xCC) {
            return "arithmetic conditioning (DAC)";
        } else if (m == 0xC4) {
            size_t q = 0;
            while (q < nb) {
                if (q + 17 > nb) return "DHT too short";
                const int tc = b[q] >> 4, th = b[q] & 15;
                if (tc != 0) return "DHT table class other than 0";
                if (th > 3) return "DHT table id above 3";
                int total = 0;
                uint32_t kraft = 0;  // in units of 2^-16
                for (int l = 1; l <= 16; ++l) {
                    const int c = b[q + l];
                    total += c;
                    kraft += (uint32_t)c << (16 - l);
                }
                if (total < 1 || total > 17) return "DHT with no value or more than 17";
                if (kraft > 65536u) return "DHT code lengths are no prefix code";
                if (q + 17 + (size_t)total > nb) return "DHT values outside the marker";
                for (int i = 0; i < 16; ++i) info->bits[th][i] = b[q + 1 + i];
                for (int i = 0; i < 17; ++i) info->values[th][i] = 0;
                for (int i = 0; i < total; ++i) {
                    const int v = b[q + 17 + i];
                    if (v > 16) return "DHT value above 16";
                    info->values[th][i] = (uint8_t)v;
                }
                info->n_values[th] = total;
                q += 17 + (size_t)total;
            }
        } else if (m == 0xDD) {
            if (nb != 2) return "DRI length";
            if (b[0] | b[1]) return "restart interval (DRI != 0)";
        } else if (m == 0xDA) {
            if (!have_sof) return "scan before the frame header";
            if (nb < 1 || b[0] != info->Nf) return "scan does not hold all components (second scan)";
            if (nb != (size_t)4 + 2 * (size_t)info->Nf) return "SOS length does not match Nf";
            for (int c = 0; c < info->Nf; ++c) {
                if (b[1 + 2 * c] != info->component_id[c]) return "scan component order";
                const int td = b[2 + 2 * c] >> 4;
                if (td > 3 || info->n_values[td] == 0) return "scan names a Huffman table that is not present";
                info->table[c] = td;
            }
            const uint8_t* t = b + 1 + 2 * info->Nf;
            info->predictor = t[0];
            info->point_transform = t[2] & 15;
            if (info->predictor < 1 || info->predictor > 7) return "predictor outside 1..7";
            if (info->point_transform != 0) return "point transform != 0";
            p += 2 + len;
            break;
        }  // APPn, COM, DQT and the rest: skipped by their length
        p += 2 + len;
    }
    // entropy-coded data: up to the first marker (FF followed by anything but 00)
    size_t e = p;
    int marker = -1;
    while (e < n) {
        if (s[e] == 0xFF) {
            if (e + 1 >= n) break;  // a lone FF at the end: the decoder ends there
            if (s[e + 1] != 0x00) {
                marker = s[e + 1];
                break;
            }
            e += 2;
        } else {
            ++e;
        }
    }
    if (marker >= 0xD0 && marker <= 0xD7) return "restart marker in the scan";
    if (marker == 0xDA || marker == 0xC4 || marker == 0xC3) return "second scan";
    if (marker >= 0 && marker != 0xD9) return "marker other than EOI behind the scan";
    if (n > 0xFFFFFFFFull) return "stream above 4 GiB";
    info->data_offset = (uint32_t)p;
    info->data_length = (uint32_t)(e - p);
    return nullptr;
}

// ---- decode table of one DHT (host) -------------------------------------------------------------------------------------
// bits[16] / values[sum(bits) <= 17] as parse() validated them -> false when they are not (no prefix code, value > 16).
inline bool build_table(const uint8_t* bits, const uint8_t* values, hhsr_ljpeg_table* t) {
    *t = hhsr_ljpeg_table{};
    int total = 0;
    uint32_t kraft = 0;
    for (int l = 1; l <= 16; ++l) {
        total += bits[l - 1];
        kraft += (uint32_t)bits[l - 1] << (16 - l);
    }
    if (total < 1 || total > 17 || kraft > 65536u) return false;
    for (int i = 0; i < total; ++i)
        if (values[i] > 16) return false;
    for (int i = 0; i < 17; ++i) t->values[i] = i < total ? values[i] : 0;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t->valoff[l] = k - code;  // values index of a code of length l = code + valoff[l]
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            if (l <= HHSR_LJPEG_LOOKUP_BITS) {
                const int lo = code << (HHSR_LJPEG_LOOKUP_BITS - l), cnt = 1 << (HHSR_LJPEG_LOOKUP_BITS - l);
                for (int j = 0; j < cnt; ++j) t->lookup[lo + j] = (uint16_t)((l << 8) | values[k]);
            }
        }
        t->maxcode[l] = bits[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[0] = -1;
    t->maxcode[17] = -1;
    return true;
}

// ---- the decoder of one stream ---------------------------------------------------------------------------------------------
// The bits of a segment's bytes, most significant first, FF 00 unstuffed; `acc` holds them left-aligned and `nbits` counts
// the real ones.  Behind the end (or a marker) zero bits follow; `starved` says that one of them was consumed.
struct BitReader {
    // The segment's bytes come from the blob as aligned little-endian dwords, four of them loaded ahead of use (w0 is
    // being consumed, w1..w3 wait): a dword's load latency is hidden behind the ~14 samples its predecessors hold.  Only
    // the dwords that hold a byte of the segment are loaded.
    const uint32_t* wp;    // the next dword to load
    const uint32_t* wend;  // behind the last dword that holds a byte of the segment
    uint32_t w0, w1, w2, w3;
    uint32_t in_w0;      // bytes left in w0
    uint32_t remaining;  // bytes of the segment not yet taken
    uint64_t acc;
    int nbits;
    bool eof, starved;

    HHSR_LJ_HD uint32_t load_next() {
        const uint32_t v = wp < wend ? *wp : 0u;
        ++wp;
        return v;
    }
    HHSR_LJ_HD void init(const uint8_t* blob, uint64_t begin, uint32_t length) {
        const uint32_t* words = (const uint32_t*)blob;
        wp = words + (begin >> 2);
        wend = words + ((begin + length + 3) >> 2);
        acc = 0;
        nbits = 0;
        remaining = length;
        eof = length == 0;
        starved = false;
        const uint32_t skip_bytes = (uint32_t)(begin & 3);
        w0 = load_next() >> (8 * skip_bytes);
        in_w0 = 4 - skip_bytes;
        w1 = load_next();
        w2 = load_next();
        w3 = load_next();
    }
    HHSR_LJ_HD uint32_t take_byte() {  // remaining > 0
        if (in_w0 == 0) {
            w0 = w1;
            w1 = w2;
            w2 = w3;
            w3 = load_next();
            in_w0 = 4;
        }
        const uint32_t b = w0 & 255u;
        w0 >>= 8;
        --in_w0;
        --remaining;
        return b;
    }
    HHSR_LJ_HD void refill() {  // at least 33 real or padding bits afterwards
        while (!eof && nbits <= 32) {
            if (in_w0 == 0) {
                w0 = w1;
                w1 = w2;
                w2 = w3;
                w3 = load_next();
                in_w0 = 4;
            }
            // the bytes of w0 that belong to the segment, next byte lowest; the others are 0
            const uint32_t k = in_w0 < remaining ? in_w0 : remaining;
            const uint32_t v = k >= 4 ? w0 : (w0 & ((1u << (8 * k)) - 1u));
            if ((((~v) - 0x01010101u) & v & 0x80808080u) == 0) {  // none of them is FF: all k at once
                const uint32_t be = (v << 24) | ((v & 0xFF00u) << 8) | ((v >> 8) & 0xFF00u) | (v >> 24);
                acc |= (uint64_t)be << (32 - nbits);
                nbits += 8 * (int)k;
                in_w0 = 0;
                remaining -= k;
            } else {  // byte by byte up to and over the FF
                const uint32_t b = take_byte();
                if (b == 0xFF) {
                    if (remaining == 0) {  // FF as the last byte: no data byte
                        eof = true;
                        break;
                    }
                    if (take_byte() != 0) {  // a marker ends the data
                        eof = true;
                        break;
                    }
                }
                acc |= (uint64_t)b << (56 - nbits);
                nbits += 8;
            }
            if (remaining == 0) eof = true;
        }
    }
    HHSR_LJ_HD uint32_t peek16() const { return (uint32_t)(acc >> 48); }
    HHSR_LJ_HD void skip(int n) {  // 0 <= n <= 16
        acc <<= n;
        nbits -= n;
        if (nbits < 0) {
            starved = true;
            nbits = 0;
        }
    }
};

// One stream into its segment of `out`: include/hhsr.h states the rules.  Returns the segment's status.  Reads
// blob[4 floor(offset / 4) .. 4 ceil((offset + length) / 4)), the tables, and reads and writes
// workspace[line_offset .. line_offset + X Nf); stores only inside the segment's rectangle clipped to the image.
HHSR_LJ_HD int32_t decode_segment(const uint8_t* blob, uint64_t blob_bytes, const hhsr_ljpeg_segment& s,
                                  const hhsr_ljpeg_table* tables, int n_tables, uint16_t* workspace,
                                  uint64_t workspace_elems, uint16_t* out, int n_frames, int H, int W, int64_t row_elems,
                                  int64_t frame_elems) {
    const int X = s.X, Y = s.Y, Nf = s.Nf;
    if (X < 1 || X > 65535 || Y < 1 || Y > 65535 || Nf < 1 || Nf > HHSR_LJPEG_MAX_COMPONENTS) return HHSR_LJPEG_BAD_SEGMENT;
    if ((int64_t)X * Y * Nf > MAX_SAMPLES) return HHSR_LJPEG_BAD_SEGMENT;
    if (s.P < 2 || s.P > 16 || s.predictor < 1 || s.predictor > 7) return HHSR_LJPEG_BAD_SEGMENT;
    if (s.offset > blob_bytes || s.length > blob_bytes - s.offset) return HHSR_LJPEG_BAD_SEGMENT;
    if (s.frame < 0 || s.frame >= n_frames || s.x0 < 0 || s.y0 < 0 || s.seg_w < 1 || s.seg_h < 1) return HHSR_LJPEG_BAD_SEGMENT;
    const uint32_t line_len = (uint32_t)(X * Nf);
    if (s.line_offset > workspace_elems || line_len > workspace_elems - s.line_offset) return HHSR_LJPEG_BAD_SEGMENT;
    const hhsr_ljpeg_table* tab[HHSR_LJPEG_MAX_COMPONENTS];
#pragma unroll
    for (int c = 0; c < HHSR_LJPEG_MAX_COMPONENTS; ++c) {  // (constant indices: the arrays stay in registers)
        const int32_t ti = c < Nf ? s.table[c] : 0;
        if (ti < 0 || ti >= n_tables) return HHSR_LJPEG_BAD_SEGMENT;
        tab[c] = tables + ti;
    }
    uint16_t* line = workspace + s.line_offset;
    const int pred = s.predictor;
    // the clipped rectangle, as counts of rows and columns of the segment that are stored
    const int rows = (int64_t)s.y0 >= H ? 0 : (s.seg_h < H - s.y0 ? s.seg_h : H - s.y0);
    const int cols = (int64_t)s.x0 >= W ? 0 : (s.seg_w < W - s.x0 ? s.seg_w : W - s.x0);
    // (an empty rectangle stores nothing: no index is formed from a y0 or x0 outside the image)
    const int64_t base = (rows > 0 && cols > 0) ? (int64_t)s.frame * frame_elems + (int64_t)s.y0 * row_elems + s.x0 : 0;

    BitReader br;
    br.init(blob, s.offset, s.length);
    int32_t left[HHSR_LJPEG_MAX_COMPONENTS] = {0, 0, 0, 0}, upleft[HHSR_LJPEG_MAX_COMPONENTS] = {0, 0, 0, 0};
    int r = 0, col = 0;  // where the next sample of the flat stream goes in the segment
    int64_t at = base;   // ... and in out, while r < rows
    for (int y = 0; y < Y; ++y) {
        for (int x = 0; x < X; ++x) {
#pragma unroll
            for (int c = 0; c < HHSR_LJPEG_MAX_COMPONENTS; ++c) {
                if (c >= Nf) break;
                br.refill();
                // Huffman code -> SSSS
                const hhsr_ljpeg_table* t = tab[c];
                const uint32_t top = br.peek16();
                const uint32_t e = t->lookup[top >> (16 - HHSR_LJPEG_LOOKUP_BITS)];
                int len = (int)(e >> 8), ssss = (int)(e & 255u);
                if (len == 0) {
                    ssss = -1;
                    for (len = HHSR_LJPEG_LOOKUP_BITS + 1; len <= 16; ++len) {
                        const int32_t code = (int32_t)(top >> (16 - len));
                        if (code <= t->maxcode[len]) {
                            const int32_t vi = code + t->valoff[len];
                            if (vi >= 0 && vi < 17) ssss = t->values[vi];
                            break;
                        }
                    }
                    if (ssss < 0) return HHSR_LJPEG_BAD_CODE;
                }
                if (len > 16 || ssss > 16) return HHSR_LJPEG_BAD_CODE;  // (a table build_table did not make)
                br.skip(len);
                // SSSS -> difference
                int32_t diff;
                if (ssss == 0) {
                    diff = 0;
                } else if (ssss == 16) {
                    diff = 32768;
                } else {
                    const int32_t v = (int32_t)(br.peek16() >> (16 - ssss));
                    br.skip(ssss);
                    diff = v < (1 << (ssss - 1)) ? v - (1 << ssss) + 1 : v;
                }
                // prediction
                const int li = x * Nf + c;
                int32_t p;
                if (y == 0) {
                    p = x == 0 ? 1 << (s.P - 1) : left[c];
                } else {
                    const int32_t Rb = (pred != 1 || x == 0) ? line[li] : 0;
                    if (x == 0) {
                        p = Rb;
                    } else {
                        const int32_t Ra = left[c], Rc = upleft[c];
                        if (pred == 1) p = Ra;  // (what DNG writers use: kept out of the switch)
                        else switch (pred) {
                            case 2: p = Rb; break;
                            case 3: p = Rc; break;
                            case 4: p = Ra + Rb - Rc; break;
                            case 5: p = Ra + ((Rb - Rc) >> 1); break;
                            case 6: p = Rb + ((Ra - Rc) >> 1); break;
                            default: p = (Ra + Rb) >> 1; break;
                        }
                    }
                    upleft[c] = Rb;
                }
                const int32_t v = (p + diff) & 0xFFFF;
                left[c] = v;
                if (pred != 1 || x == 0) line[li] = (uint16_t)v;  // (predictor 1 reads the line above in column 0 only)
                if (r < rows && col < cols) out[at + col] = (uint16_t)v;
                if (++col == s.seg_w) {
                    col = 0;
                    if (r < rows) {  // (rows <= seg_h: behind it nothing is stored, and r stays bounded)
                        ++r;
                        at += row_elems;
                    }
                }
            }
        }
    }
    return br.starved ? HHSR_LJPEG_TRUNCATED : HHSR_LJPEG_OK;
}

// hhsr_ljpeg_workspace's rule: the line buffers one after the other.  false when they pass 2^32 elements.
inline bool assign_workspace(hhsr_ljpeg_segment* segs, int n, size_t* bytes) {
    uint64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t X = segs[i].X, Nf = segs[i].Nf;
        if (X < 1 || X > 65535 || Nf < 1 || Nf > HHSR_LJPEG_MAX_COMPONENTS) return false;
        segs[i].line_offset = (uint32_t)at;
        at += (uint64_t)(X * Nf);
        if (at > 0xFFFFFFFFull) return false;
    }
    *bytes = (size_t)(at * sizeof(uint16_t));
    return true;
}

}  // namespace hhsr_lj
