// PNG output, the part that needs no device (include/hhsr.h "PNG output"): the geometry of a file, counts -> the optimal
// length-limited code (package-merge) and the dynamic-Huffman block header (RFC 1951 3.2.7), canonical code words, the
// CRC-32 algebra (remainders of pieces -> the CRC of their concatenation) and the writers of the file's fixed parts.
// Plain C++17 without a HIP include, so that a stand-alone program can compile it under a sanitiser; hhsr_png.hip wraps it
// in the C ABI.
#ifndef HHSR_PNG_TABLES_H
#define HHSR_PNG_TABLES_H
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define PNG_HD __host__ __device__
#else
#define PNG_HD
#endif

namespace png {
constexpr int N_SYM = 257;             // literals 0 .. 255 and the end-of-block symbol 256
constexpr int MAX_LEN = 15;            // RFC 1951: a literal/length code has at most 15 bits
constexpr int SPEC_LEN_AT = 0;         // spec: lengths[257] | 0 | header bits (uint16, little-endian) | header bit string
constexpr int SPEC_BITS_AT = 258;
constexpr int SPEC_HDR_AT = 260;
constexpr int SPEC_BYTES = 768;        // HHSR_PNG_SPEC_BYTES
constexpr int HDR_WORDS = 127;         // the header as a kernel argument: at most 4064 bits
// 3 (BFINAL, BTYPE) + 14 (HLIT, HDIST, HCLEN) + 19 x 3 + 259 code lengths of at most 7 bits + 7 extra bits each
constexpr int HDR_MAX_BITS = 17 + 57 + 259 * 14;
static_assert(HDR_MAX_BITS <= HDR_WORDS * 32 && HDR_MAX_BITS <= (SPEC_BYTES - SPEC_HDR_AT) * 8, "header storage");
constexpr uint32_t MAX_INTERVAL = 1u << 20;
constexpr int SCAN_GROUP = 2048;       // intervals per workgroup of the offsets scan (= jpeg::SCAN_GROUP, asserted in hhsr_png.hip)
constexpr int FILTER_MAX_GROUPS = 1024;  // k_png_filter: persistent workgroups, one partial count table each
constexpr uint32_t ADLER_MOD = 65521;

// ---- CRC-32 (ISO 3309, the reflected polynomial 0xEDB88320) as polynomial arithmetic modulo P ------------------------------
// A 32-bit word holds a polynomial with the coefficient of x^0 in bit 31.  raw(M) = M(x) x^32 mod P is what the table-driven
// update computes from a zero register; raw(A | B) = raw(A) x^(8 len B) + raw(B), and
// crc32(M) = raw(M) + 0xFFFFFFFF x^(8 len M) + 0xFFFFFFFF.
constexpr uint32_t CRC_POLY = 0xEDB88320u;

PNG_HD constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {  // a b mod P
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

struct CrcPowers {
    uint32_t x2n[32];  // x^(2^k) mod P; the sequence has period 32 in k (x^(2^32) = x)
};
constexpr CrcPowers crc_powers() {
    CrcPowers t{};
    uint32_t p = 0x40000000u;  // x^1
    for (int k = 0; k < 32; ++k) {
        t.x2n[k] = p;
        p = crc_mul(p, p);
    }
    return t;
}

PNG_HD constexpr uint32_t crc_xpow8(uint64_t n, const uint32_t* x2n) {  // x^(8 n) mod P
    uint32_t p = 0x80000000u;  // x^0
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1u) p = crc_mul(x2n[k & 31], p);
    return p;
}

PNG_HD constexpr uint32_t crc_byte(uint32_t r, uint32_t byte) {  // the register after one more byte (no table)
    r ^= byte;
    for (int k = 0; k < 8; ++k) r = (r & 1u) ? (r >> 1) ^ CRC_POLY : r >> 1;
    return r;
}

// v -> v x^2048 mod P as four 256-entry tables (one per byte of v): a lane of the coder that owns every 64th 32-bit word
// of an interval advances its register by 256 bytes per word with four look-ups
struct CrcStride {
    uint32_t t[4][256];
};
constexpr CrcStride crc_stride() {
    CrcStride s{};
    const CrcPowers pw = crc_powers();
    const uint32_t x2048 = pw.x2n[11];
    // linear: the images of the 32 unit vectors, then every byte value as the sum over its set bits
    uint32_t unit[32] = {};
    for (int b = 0; b < 32; ++b) unit[b] = crc_mul(1u << b, x2048);
    for (int k = 0; k < 4; ++k)
        for (int v = 0; v < 256; ++v) {
            uint32_t r = 0;
            for (int b = 0; b < 8; ++b)
                if (v >> b & 1) r ^= unit[8 * k + b];
            s.t[k][v] = r;
        }
    return s;
}

inline uint32_t crc32_bytes(const uint8_t* p, size_t n, uint32_t crc = 0) {  // zlib's crc32(crc, p, n)
    uint32_t r = ~crc;
    for (size_t i = 0; i < n; ++i) r = crc_byte(r, p[i]);
    return ~r;
}

// crc32(A | B) from crc32(A), crc32(B) and len B (the pre- and post-conditioning cancel: zlib's crc32_combine)
inline uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    constexpr CrcPowers pw = crc_powers();
    return crc_mul(crc_xpow8(len_b, pw.x2n), crc_a) ^ crc_b;  // (any len_b: the powers wrap with their period)
}

// ---- geometry -------------------------------------------------------------------------------------------------------------
struct Geom {
    size_t row_bytes, stream_bytes, n_int, n_groups, filter_groups;
    size_t scratch_filter, scratch_deflate, scratch_bytes, max_deflate;
    int bpp;
};

// false: the filtered stream or its bound does not fit 2^31 - 1 bytes (one IDAT chunk)
inline bool geom(int H, int W, int och, int bits, uint32_t interval, Geom* g) {
    g->bpp = och * bits / 8;
    const uint64_t row = (uint64_t)W * g->bpp, n = (uint64_t)H * (1 + row);
    if (n > 0x7fffffffull) return false;
    g->row_bytes = (size_t)row;
    g->stream_bytes = (size_t)n;
    g->n_int = (size_t)((n + interval - 1) / interval);
    g->n_groups = (g->n_int + SCAN_GROUP - 1) / SCAN_GROUP;
    g->filter_groups = (size_t)H < (size_t)FILTER_MAX_GROUPS ? (size_t)H : (size_t)FILTER_MAX_GROUPS;
    g->scratch_filter = g->filter_groups * 256 * sizeof(uint32_t);
    // uint64 offsets[n_int] | uint64 group totals[n_groups] | uint32 sizes, crc, adler s1, adler s2 [n_int] each
    g->scratch_deflate = (g->n_int + g->n_groups) * sizeof(uint64_t) + 4 * g->n_int * sizeof(uint32_t);
    g->scratch_bytes = g->scratch_filter > g->scratch_deflate ? g->scratch_filter : g->scratch_deflate;
    // The bound (derived in include/hhsr.h): T = N + n_int coded symbols cost at most 8 T + 2 T / 257 + 1 bits; an interval
    // adds its header, the 3 bits of the empty stored block, fewer than 8 bits of padding twice, and 4 bytes of marker.
    const uint64_t t = n + g->n_int;
    const uint64_t data_bits = 8 * t + 2 * t / 257 + 1;
    const uint64_t per_int = (HDR_MAX_BITS + 3 + 7) / 8 + 1 + 4;
    const uint64_t bound = (data_bits + 7) / 8 + g->n_int * per_int;
    if (bound > 0x7fffffffull) return false;
    g->max_deflate = (size_t)bound;
    return true;
}

// ---- length-limited optimal codes: package-merge (Larmore & Hirschberg 1990) ---------------------------------------------------
// counts[n] -> lens[n]: a zero count gets length 0; the others a complete prefix code of lengths <= limit that minimises
// sum count x length.  false: fewer than 2 counted symbols, more than 2^limit of them, or counts that sum to 2^59 or more.
// n <= 288.  The items of a level are the leaves (ascending count, then symbol) merged with the packages of the level
// below (pairs of its consecutive items), a leaf before a package of the same weight; a symbol's length is the number of
// the first 2 m - 2 items of the top level that contain its leaf.
inline bool package_merge(const uint64_t* counts, int n, int limit, uint8_t* lens) {
    constexpr int MAXN = 288;
    if (n > MAXN) return false;
    int order[MAXN], m = 0;
    uint64_t total = 0;
    for (int s = 0; s < n; ++s) {
        lens[s] = 0;
        if (counts[s]) {
            if (counts[s] >= (1ull << 59) || total + counts[s] >= (1ull << 59)) return false;  // (an item weighs at most limit x total)
            total += counts[s];
            order[m++] = s;
        }
    }
    if (m < 2 || (limit < 31 && m > (1 << limit))) return false;
    for (int i = 1; i < m; ++i) {  // insertion sort by (count, symbol): m <= 288
        const int s = order[i];
        int j = i;
        for (; j > 0 && counts[order[j - 1]] > counts[s]; --j) order[j] = order[j - 1];
        order[j] = s;
    }
    // an item: its weight and how many leaves of every rank it contains (<= limit each)
    struct Item {
        uint64_t w;
        uint8_t k[MAXN];
    };
    const int cap = 2 * m;
    Item* prev = new Item[cap];
    Item* cur = new Item[cap];
    int n_prev = 0;
    for (int level = 0; level < limit; ++level) {
        int n_cur = 0, leaf = 0, pk = 0;
        const int n_pk = n_prev / 2;
        while (leaf < m || pk < n_pk) {
            const uint64_t wl = leaf < m ? counts[order[leaf]] : 0;
            uint64_t wp = 0;
            if (pk < n_pk) wp = prev[2 * pk].w + prev[2 * pk + 1].w;
            const bool take_leaf = leaf < m && (pk >= n_pk || wl <= wp);
            Item& it = cur[n_cur++];
            if (take_leaf) {
                it.w = wl;
                for (int r = 0; r < m; ++r) it.k[r] = 0;
                it.k[leaf++] = 1;
            } else {
                it.w = wp;
                for (int r = 0; r < m; ++r) it.k[r] = (uint8_t)(prev[2 * pk].k[r] + prev[2 * pk + 1].k[r]);
                ++pk;
            }
            if (n_cur == cap) break;  // (only the first 2 m - 2 items of a level are ever used)
        }
        Item* t = prev;
        prev = cur;
        cur = t;
        n_prev = n_cur;
    }
    for (int i = 0; i < 2 * m - 2; ++i)
        for (int r = 0; r < m; ++r) lens[order[r]] = (uint8_t)(lens[order[r]] + prev[i].k[r]);
    delete[] prev;
    delete[] cur;
    return true;
}

// canonical code words of RFC 1951 3.2.2, bit-reversed (a Huffman code goes into the LSB-first stream MSB first):
// out[s] = reversed code | length << 16
inline void canonical_reversed(const uint8_t* lens, int n, uint32_t* out) {
    uint32_t bl_count[MAX_LEN + 1] = {}, next_code[MAX_LEN + 2] = {};
    for (int s = 0; s < n; ++s) ++bl_count[lens[s]];
    bl_count[0] = 0;
    uint32_t code = 0;
    for (int b = 1; b <= MAX_LEN; ++b) {
        code = (code + bl_count[b - 1]) << 1;
        next_code[b] = code;
    }
    for (int s = 0; s < n; ++s) {
        const int len = lens[s];
        uint32_t rev = 0;
        if (len) {
            const uint32_t c = next_code[len]++;
            for (int b = 0; b < len; ++b) rev |= (c >> b & 1u) << (len - 1 - b);
        }
        out[s] = rev | (uint32_t)len << 16;
    }
}

// sum 2^-len over the coded symbols, in units of 2^-15: a complete code gives exactly 2^15
inline uint32_t kraft15(const uint8_t* lens, int n) {
    uint32_t k = 0;
    for (int s = 0; s < n; ++s)
        if (lens[s]) k += 1u << (MAX_LEN - lens[s]);
    return k;
}

struct BitWriter {  // LSB-first, into a zeroed buffer
    uint8_t* p;
    size_t cap_bits, n = 0;
    bool ok = true;
    void put(uint32_t v, int count) {
        for (int b = 0; b < count; ++b, ++n) {
            if (n >= cap_bits) {
                ok = false;
                return;
            }
            p[n >> 3] = (uint8_t)(p[n >> 3] | (v >> b & 1u) << (n & 7));
        }
    }
};

// counts[257] -> spec: the lengths, and the header of a dynamic-Huffman block with BFINAL 0: BTYPE 10, HLIT 257 codes,
// HDIST 2 codes of length 1, the 259 lengths run-length coded (17 and 18 for runs of zeros; 16 is not used) under an
// optimal code of at most 7 bits for the code-length alphabet.
inline bool build_spec(const uint64_t* counts, uint8_t* spec) {
    uint8_t lens[N_SYM];
    if (!counts[256]) return false;  // every block ends
    bool any_byte = false;
    for (int s = 0; s < 256; ++s) any_byte |= counts[s] != 0;
    if (!any_byte || !package_merge(counts, N_SYM, MAX_LEN, lens)) return false;
    for (int i = 0; i < SPEC_BYTES; ++i) spec[i] = 0;
    for (int s = 0; s < N_SYM; ++s) spec[SPEC_LEN_AT + s] = lens[s];
    uint8_t seq[N_SYM + 2];
    for (int s = 0; s < N_SYM; ++s) seq[s] = lens[s];
    seq[N_SYM] = seq[N_SYM + 1] = 1;
    // run-length symbols: (symbol, extra bits value)
    uint8_t sym[N_SYM + 2], extra[N_SYM + 2];
    int n_sym = 0;
    for (int i = 0; i < N_SYM + 2;) {
        int run = 1;
        if (seq[i] == 0)
            while (i + run < N_SYM + 2 && seq[i + run] == 0 && run < 138) ++run;
        if (seq[i] == 0 && run >= 11) {
            sym[n_sym] = 18, extra[n_sym++] = (uint8_t)(run - 11);
        } else if (seq[i] == 0 && run >= 3) {
            sym[n_sym] = 17, extra[n_sym++] = (uint8_t)(run - 3);
        } else {
            run = 1;
            sym[n_sym] = seq[i], extra[n_sym++] = 0;
        }
        i += run;
    }
    uint64_t cl_counts[19] = {};
    for (int i = 0; i < n_sym; ++i) ++cl_counts[sym[i]];
    uint8_t cl_lens[19];
    if (!package_merge(cl_counts, 19, 7, cl_lens)) return false;  // (at least the lengths 1 of HDIST and one other symbol)
    uint32_t cl_codes[19];
    canonical_reversed(cl_lens, 19, cl_codes);
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 19;
    while (hclen > 4 && cl_lens[order[hclen - 1]] == 0) --hclen;
    BitWriter w{spec + SPEC_HDR_AT, (size_t)HDR_MAX_BITS};
    w.put(0, 1);           // BFINAL: set by the coder in the last interval
    w.put(2, 2);           // BTYPE 10
    w.put(N_SYM - 257, 5);  // HLIT
    w.put(2 - 1, 5);       // HDIST
    w.put((uint32_t)hclen - 4, 4);
    for (int i = 0; i < hclen; ++i) w.put(cl_lens[order[i]], 3);
    for (int i = 0; i < n_sym; ++i) {
        w.put(cl_codes[sym[i]] & 0xffffu, (int)(cl_codes[sym[i]] >> 16));
        if (sym[i] == 17) w.put(extra[i], 3);
        if (sym[i] == 18) w.put(extra[i], 7);
    }
    if (!w.ok) return false;
    spec[SPEC_BITS_AT] = (uint8_t)(w.n & 0xff);
    spec[SPEC_BITS_AT + 1] = (uint8_t)(w.n >> 8);
    return true;
}

// what the coder takes with a launch: code words, the header as words
struct Codes {
    uint32_t code[N_SYM];  // reversed code | length << 16
    uint32_t hdr_bits;
    uint32_t hdr[HDR_WORDS];
};

// false: lengths above 15, a code that is not complete, no end-of-block code, a header of impossible length or BFINAL set
inline bool codes_from_spec(const uint8_t* spec, Codes* c) {
    const uint8_t* lens = spec + SPEC_LEN_AT;
    for (int s = 0; s < N_SYM; ++s)
        if (lens[s] > MAX_LEN) return false;
    if (kraft15(lens, N_SYM) != (1u << MAX_LEN) || lens[256] == 0 || spec[257] != 0) return false;
    const uint32_t bits = spec[SPEC_BITS_AT] | (uint32_t)spec[SPEC_BITS_AT + 1] << 8;
    if (bits < 17 + 4 * 3 || bits > (uint32_t)HDR_MAX_BITS) return false;
    if ((spec[SPEC_HDR_AT] & 7) != 4) return false;  // BFINAL 0, BTYPE 10
    canonical_reversed(lens, N_SYM, c->code);
    c->hdr_bits = bits;
    for (int i = 0; i < HDR_WORDS; ++i) c->hdr[i] = 0;
    for (uint32_t b = 0; b < bits; ++b) c->hdr[b >> 5] |= (uint32_t)(spec[SPEC_HDR_AT + (b >> 3)] >> (b & 7) & 1u) << (b & 31);
    return true;
}

// ---- the file's fixed parts -----------------------------------------------------------------------------------------------------
inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}
constexpr size_t HEAD_BYTES = 8 + 25 + 8 + 2;  // signature, IHDR chunk, IDAT length and type, 78 01
constexpr size_t TAIL_BYTES = 4 + 4 + 12;      // Adler-32, IDAT CRC, IEND chunk

inline void file_head(int H, int W, int och, int bits, uint32_t deflate_len, uint8_t* b) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int i = 0; i < 8; ++i) b[i] = sig[i];
    put_be32(b + 8, 13);
    b[12] = 'I', b[13] = 'H', b[14] = 'D', b[15] = 'R';
    put_be32(b + 16, (uint32_t)W);
    put_be32(b + 20, (uint32_t)H);
    b[24] = (uint8_t)bits, b[25] = och == 3 ? 2 : 0, b[26] = 0, b[27] = 0, b[28] = 0;
    put_be32(b + 29, crc32_bytes(b + 12, 17));
    put_be32(b + 33, deflate_len + 6);  // 78 01, the deflate stream, the Adler-32
    b[37] = 'I', b[38] = 'D', b[39] = 'A', b[40] = 'T';
    b[41] = 0x78, b[42] = 0x01;
}

inline void file_tail(uint32_t deflate_crc, uint64_t deflate_len, uint32_t adler, uint8_t* b) {
    static const uint8_t lead[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    put_be32(b, adler);
    uint32_t crc = crc_combine(crc32_bytes(lead, 6), deflate_crc, deflate_len);
    crc = crc_combine(crc, crc32_bytes(b, 4), 4);
    put_be32(b + 4, crc);
    put_be32(b + 8, 0);
    b[12] = 'I', b[13] = 'E', b[14] = 'N', b[15] = 'D';
    put_be32(b + 16, crc32_bytes(b + 12, 4));
}
}  // namespace png
#endif  // HHSR_PNG_TABLES_H
