// The host core of the lossless-JPEG encoder under sanitizers, as a stand-alone program (tests/test_ljpeg_enc_host.py builds
// it with clang++ -fsanitize=address,undefined and runs it as a child process):
//   ljpeg_enc_main
// Every edge case is encoded by hhsr_lje::encode_image into a buffer inside guard bands, at full and at cut capacity; the
// tiles are decoded again by hhsr_lj::decode_segment and compared with the image; the guards are checked.  It includes the
// host cores only: no HIP, no library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../handheld-multi-frame-super-resolution_amd/csrc/hhsr_ljpeg_core.h"
#include "../handheld-multi-frame-super-resolution_amd/csrc/hhsr_ljpeg_enc_core.h"

namespace lje = hhsr_lje;

static const uint8_t GUARD = 0xA5;
static const size_t BAND = 64;
static int failures = 0;

#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            printf("FAILED: " __VA_ARGS__); \
            printf("\n");                \
            ++failures;                  \
        }                                \
    } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

enum Kind { NOISE, FLAT, ALT, SMOOTH };

static void run_case(const char* name, Kind kind, int H, int W, int Nf, int P, int predictor, int th, int tw, int pad) {
    const int64_t row = (int64_t)W * Nf + pad;
    std::vector<uint16_t> img((size_t)(H * row), 0xBEEF);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < Nf; ++c) {
                uint32_t v;
                switch (kind) {
                    case NOISE: v = rnd(); break;
                    case FLAT: v = 1u << (P - 1); break;
                    case ALT: v = (x & 1) ? 0u : 32768u; break;
                    default: v = (uint32_t)(y * 37 + x * 53 + c * 11) + rnd() % 6; break;
                }
                img[(size_t)(y * row + (int64_t)x * Nf + c)] = (uint16_t)(v & ((1u << P) - 1u));
            }
    lje::Geom g;
    if (!lje::geom(H, W, Nf, th, tw, &g)) {
        CHECK(false, "%s: geom", name);
        return;
    }
    // counts -> tables
    std::vector<uint64_t> counts((size_t)Nf * 17, 0);
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx)
            for (int y = 0; y < th; ++y)
                for (int x = 0; x < tw; ++x)
                    for (int c = 0; c < Nf; ++c) {
                        auto s = [&](int yy, int xx) { return lje::tile_sample(img.data(), H, W, Nf, row, ty * th, tx * tw, yy, xx, c); };
                        const int32_t p = lje::predict(predictor, P, y, x, x ? s(y, x - 1) : 0, y ? s(y - 1, x) : 0,
                                                       x && y ? s(y - 1, x - 1) : 0);
                        int32_t d;
                        ++counts[(size_t)c * 17 + lje::category(s(y, x), p, &d)];
                    }
    std::vector<uint8_t> bits((size_t)Nf * 16), values((size_t)Nf * 17);
    for (int c = 0; c < Nf; ++c) {
        int n;
        CHECK(lje::build_k2(&counts[(size_t)c * 17], &bits[(size_t)c * 16], &values[(size_t)c * 17], &n), "%s: build_k2", name);
    }
    lje::Codes codes;
    CHECK(lje::make_codes(bits.data(), values.data(), Nf, P, predictor, th, tw, &codes), "%s: make_codes", name);

    std::vector<uint64_t> offsets(g.n_tiles + 1), offsets_cut(g.n_tiles + 1);
    std::vector<uint32_t> tile_bytes(g.n_tiles), tile_bytes_cut(g.n_tiles);
    uint64_t length = 0;
    std::vector<uint8_t> whole(BAND + g.max_bytes + BAND, GUARD);
    lje::encode_image(img.data(), H, W, Nf, row, P, predictor, th, tw, codes, g, whole.data() + BAND, g.max_bytes, offsets.data(),
                      tile_bytes.data(), &length);
    CHECK(length != UINT64_MAX && length <= g.max_bytes, "%s: length %llu above the bound %llu", name,
          (unsigned long long)length, (unsigned long long)g.max_bytes);
    if (length == UINT64_MAX || length > g.max_bytes) return;
    for (size_t i = 0; i < BAND; ++i) CHECK(whole[i] == GUARD, "%s: guard in front", name);
    for (size_t i = BAND + length; i < whole.size(); ++i) CHECK(whole[i] == GUARD, "%s: byte %zu behind the result written", name, i);

    // cut capacities: exact heap blocks, so that the sanitizer sees a byte too many as well
    const uint64_t caps[] = {length / 2, length / 2 + 1, 0, 1, length - 1, length};
    for (uint64_t cap : caps) {
        uint8_t* cut = (uint8_t*)malloc(cap ? cap : 1);
        uint64_t len_cut = 0;
        lje::encode_image(img.data(), H, W, Nf, row, P, predictor, th, tw, codes, g, cut, cap, offsets_cut.data(),
                          tile_bytes_cut.data(), &len_cut);
        CHECK(len_cut == length && offsets_cut == offsets && tile_bytes_cut == tile_bytes, "%s: cut at %llu changes the record",
              name, (unsigned long long)cap);
        CHECK(memcmp(cut, whole.data() + BAND, cap) == 0, "%s: cut at %llu is no prefix", name, (unsigned long long)cap);
        free(cut);
    }

    // decode every tile again
    std::vector<uint16_t> back((size_t)(H * row), 0xBEEF), line((size_t)tw * Nf);
    for (uint64_t t = 0; t < g.n_tiles; ++t) {
        const uint8_t* s = whole.data() + BAND + offsets[t];
        CHECK((offsets[t] & 1) == 0 && offsets[t + 1] == offsets[t] + tile_bytes[t] + (tile_bytes[t] & 1), "%s: layout", name);
        hhsr_ljpeg_info info;
        const char* why = hhsr_lj::parse(s, tile_bytes[t], &info);
        CHECK(why == nullptr, "%s: tile %llu refused: %s", name, (unsigned long long)t, why ? why : "");
        if (why) continue;
        CHECK(info.X == tw && info.Y == th && info.Nf == Nf && info.P == P && info.predictor == predictor, "%s: header", name);
        hhsr_ljpeg_table tabs[4];
        for (int c = 0; c < Nf; ++c) CHECK(hhsr_lj::build_table(info.bits[info.table[c]], info.values[info.table[c]], &tabs[c]), "%s: table", name);
        // the entropy-coded bytes in a 4-byte aligned blob of their own
        std::vector<uint32_t> blob((info.data_length + 3) / 4 + 1, 0);
        memcpy(blob.data(), s + info.data_offset, info.data_length);
        hhsr_ljpeg_segment seg{};
        seg.offset = 0, seg.length = info.data_length, seg.line_offset = 0;
        seg.X = tw, seg.Y = th, seg.Nf = Nf, seg.P = P, seg.predictor = predictor;
        for (int c = 0; c < Nf; ++c) seg.table[c] = c;
        seg.frame = 0, seg.x0 = (int)(t % g.tiles_x) * tw * Nf, seg.y0 = (int)(t / g.tiles_x) * th, seg.seg_w = tw * Nf, seg.seg_h = th;
        const int32_t st = hhsr_lj::decode_segment((const uint8_t*)blob.data(), ((uint64_t)info.data_length + 3) / 4 * 4, seg, tabs, Nf,
                                                   line.data(), line.size(), back.data(), 1, H, W * Nf, row, (int64_t)H * row);
        CHECK(st == HHSR_LJPEG_OK, "%s: tile %llu decodes with status %d", name, (unsigned long long)t, st);
    }
    CHECK(back == img, "%s: the decoded image differs (or a pad element was written)", name);
    printf("%-28s %4d x %4d x %d  P %2d  predictor %d  %llu tiles  %llu bytes\n", name, H, W, Nf, P, predictor,
           (unsigned long long)g.n_tiles, (unsigned long long)length);
}

int main() {
    for (int predictor = 1; predictor <= 7; ++predictor) run_case("edge tiles", SMOOTH, 40, 56, 3, 16, predictor, 16, 32, 5);
    run_case("one component", SMOOTH, 40, 56, 1, 16, 1, 16, 32, 0);
    run_case("precision 10", SMOOTH, 40, 56, 3, 10, 1, 16, 32, 1);
    run_case("two components", NOISE, 17, 33, 2, 12, 4, 16, 16, 0);
    run_case("four components", NOISE, 16, 16, 4, 16, 7, 16, 16, 0);
    run_case("flat", FLAT, 32, 32, 1, 16, 1, 16, 16, 0);
    run_case("alternating 0 / 32768", ALT, 16, 32, 1, 16, 1, 16, 32, 0);
    run_case("full-range noise", NOISE, 40, 56, 3, 16, 1, 16, 32, 0);
    run_case("one pixel", NOISE, 1, 1, 3, 16, 6, 16, 16, 0);
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("guards intact\n");
    return 0;
}
