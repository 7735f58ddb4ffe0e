// Stand-alone driver of csrc/hhsr_jpeg_tables.h (the JPEG table construction and header writer: no HIP in them), built by
// tests/test_jpeg_ex_host.py with g++ -fsanitize=address,undefined.  Every buffer is a heap allocation of exactly the
// length the contract states.  One request per input line, one answer per output line:
//   huffman c0 .. c255                                     -> spec <544 hex digits> | refused
//   header H W components quality restart sub <hex spec|-> -> header <hex> | refused
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hhsr_jpeg_tables.h"

static void print_hex(const char* tag, const uint8_t* p, size_t n) {
    std::printf("%s ", tag);
    for (size_t i = 0; i < n; ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "huffman") {
            std::vector<uint64_t> counts(256);
            for (auto& c : counts) in >> c;
            std::vector<uint8_t> spec(jpeg::SPEC_BYTES, 0xA5);
            if (!in || !jpeg::huffman_build(counts.data(), spec.data())) {
                std::printf("refused\n");
                continue;
            }
            jpeg::HuffSpec parsed;  // what was built must be a table the header and the coder accept
            if (!jpeg::spec_parse(spec.data(), false, &parsed)) {
                std::printf("built an invalid table\n");
                return 1;
            }
            print_hex("spec", spec.data(), spec.size());
        } else if (what == "header") {
            int H, W, nc, quality, restart, sub;
            std::string hex;
            in >> H >> W >> nc >> quality >> restart >> sub >> hex;
            const int n_tables = nc == 1 ? 2 : 4;
            std::vector<uint8_t> spec;
            if (hex != "-") {
                for (size_t i = 0; i + 1 < hex.size(); i += 2) spec.push_back((uint8_t)std::stoi(hex.substr(i, 2), nullptr, 16));
                if (spec.size() != (size_t)n_tables * jpeg::SPEC_BYTES) return 2;
            }
            jpeg::HuffSpec store[4];
            const jpeg::HuffSpec* specs[4];
            if (!in || !jpeg::specs_from_abi(spec.empty() ? nullptr : spec.data(), n_tables, store, specs)) {
                std::printf("refused\n");
                continue;
            }
            size_t need = 0;
            std::vector<uint8_t> none(1);
            if (jpeg::write_header(H, W, nc, quality, restart, sub, specs, none.data(), 0, &need) != 1) return 3;
            std::vector<uint8_t> out(need);  // exactly the reported length
            if (jpeg::write_header(H, W, nc, quality, restart, sub, specs, out.data(), out.size(), &need) != 0) return 4;
            const jpeg::HuffCodes codes = jpeg::huff_codes(specs);  // annex C over the same tables
            unsigned filled = 0;
            for (int i = 0; i < jpeg::HUFF_WORDS; ++i) filled += reinterpret_cast<const uint32_t*>(&codes)[i] != 0;
            std::printf("codes %u ", filled);
            print_hex("header", out.data(), out.size());
        } else if (!what.empty()) {
            return 5;
        }
    }
    return 0;
}
