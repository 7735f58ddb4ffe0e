/* Plain-C client of libhhsr_hip.so: no Python, no torch — the drop-in boundary is the C ABI of include/hhsr.h.
 *
 *   gcc -std=c11 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/hhsr_c_demo.c \
 *       -Lhandheld-multi-frame-super-resolution_amd/handheld_super_resolution -lhhsr_hip \
 *       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$ORIGIN' -o hhsr_c_demo
 *
 * Normalises a synthetic uint16 Bayer frame (hhsr_normalize_raw_u16), builds one Gaussian pyramid level
 * (hhsr_gauss_decimate), encodes the frame as uint8 / uint16 samples (hhsr_encode_image) and checks all three against the
 * same arithmetic done on the host; then codes the frame as a baseline JPEG (hhsr_jpeg_header, _workspace, _dct, _entropy)
 * and, given a path as its argument, writes the file there.  Exit code 0 = match. */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hhsr.h"

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define CHECK_HHSR(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, hhsr_last_error()); return 3; } } while (0)

int main(int argc, char** argv) {
    enum { H = 64, W = 96, F = 2, NT = 4 * F + 1 };
    static uint16_t counts[H * W];
    static float norm_host[H * W], norm_dev[H * W];
    const uint8_t cfa[4] = {0, 1, 1, 2};
    const double black[3] = {64, 64, 64}, wb[3] = {1.9, 1.0, 1.6};
    const double white = 4095;
    for (int i = 0; i < H * W; ++i) counts[i] = (uint16_t)(64 + (i * 2654435761u >> 20) % 4000);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int c = cfa[(y & 1) * 2 + (x & 1)];
            const float v = ((float)counts[y * W + x] - (float)black[c]) / (float)(white - black[c]);
            norm_host[y * W + x] = v * (float)(wb[c] / wb[1]);
        }
    printf("%s\n", hhsr_version());
    uint16_t* d_counts;
    float *d_norm, *d_lvl;
    CHECK_HIP(hipMalloc((void**)&d_counts, sizeof counts));
    CHECK_HIP(hipMalloc((void**)&d_norm, sizeof norm_dev));
    CHECK_HIP(hipMemcpy(d_counts, counts, sizeof counts, hipMemcpyHostToDevice));
    CHECK_HHSR(hhsr_normalize_raw_u16(d_counts, 1, H, W, W, cfa, black, white, wb, d_norm, NULL));
    CHECK_HIP(hipMemcpy(norm_dev, d_norm, sizeof norm_dev, hipMemcpyDeviceToHost));
    for (int i = 0; i < H * W; ++i)
        if (norm_dev[i] != norm_host[i]) { fprintf(stderr, "normalise mismatch at %d: %g vs %g\n", i, norm_dev[i], norm_host[i]); return 1; }

    /* one pyramid level: 9-tap Gaussian (sigma = 1), valid convolution, decimate by 2 */
    float taps[NT], sum = 0.f;
    for (int k = 0; k < NT; ++k) { taps[k] = expf(-0.5f * (float)((k - 4) * (k - 4))); sum += taps[k]; }
    for (int k = 0; k < NT; ++k) taps[k] /= sum;
    const int h2 = (H - 8) / F, w2 = (W - 8) / F;
    CHECK_HIP(hipMalloc((void**)&d_lvl, sizeof(float) * h2 * w2));
    CHECK_HHSR(hhsr_gauss_decimate(d_norm, H, W, W, d_lvl, w2, F, taps, NT, NULL));
    float* lvl = (float*)malloc(sizeof(float) * h2 * w2);
    CHECK_HIP(hipMemcpy(lvl, d_lvl, sizeof(float) * h2 * w2, hipMemcpyDeviceToHost));
    double worst = 0;
    for (int y = 0; y < h2; ++y)
        for (int x = 0; x < w2; ++x) {
            double acc = 0;
            for (int j = 0; j < NT; ++j) {
                double col = 0;
                for (int i = 0; i < NT; ++i) col += (double)taps[i] * norm_host[(y * F + i) * W + x * F + j];
                acc += (double)taps[j] * col;
            }
            const double d = fabs(acc - lvl[y * w2 + x]);
            if (d > worst) worst = d;
        }
    printf("normalise: bit-exact; pyramid level %dx%d: max abs diff vs float64 %.2e\n", h2, w2, worst);
    /* integer output: the normalised frame (values up to 1.9: clipped) as uint8 with padded rows from an odd base, and
     * as compact uint16, against the rule of hhsr.h written out on the host */
    enum { ROW8 = W + 5, OFF8 = 3 };
    static uint8_t enc8[OFF8 + H * ROW8];
    static uint16_t enc16[H * W];
    uint8_t* d_enc8;
    uint16_t* d_enc16;
    CHECK_HIP(hipMalloc((void**)&d_enc8, sizeof enc8));
    CHECK_HIP(hipMalloc((void**)&d_enc16, sizeof enc16));
    CHECK_HIP(hipMemset(d_enc8, 0xA5, sizeof enc8));
    CHECK_HHSR(hhsr_encode_image(d_norm, H, W, 1, 1, d_enc8 + OFF8, 8, ROW8, NULL));
    CHECK_HHSR(hhsr_encode_image(d_norm, H, W, 1, 1, d_enc16, 16, W * sizeof(uint16_t), NULL));
    CHECK_HIP(hipMemcpy(enc8, d_enc8, sizeof enc8, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(enc16, d_enc16, sizeof enc16, hipMemcpyDeviceToHost));
    for (int i = 0; i < OFF8 + H * ROW8; ++i) {
        const int y = (i - OFF8) / ROW8, x = (i - OFF8) % ROW8;
        unsigned want = 0xA5; /* in front of the base, between the rows: untouched */
        if (i >= OFF8 && x < W) {
            float v = norm_host[y * W + x];
            v = v != v ? 0.f : (v < 0.f ? 0.f : (v > 1.f ? 1.f : v));
            want = (unsigned)rintf(v * 255.f); /* half to even */
            if (enc16[y * W + x] != (unsigned)rintf(v * 65535.f)) { fprintf(stderr, "uint16 mismatch at %d,%d\n", y, x); return 1; }
        }
        if (enc8[i] != want) { fprintf(stderr, "uint8 mismatch at byte %d: %u vs %u\n", i, enc8[i], want); return 1; }
    }
    printf("encode: uint8 (rows of %d bytes from base + %d) and uint16 match the host rule, padding untouched\n", ROW8, OFF8);
    hipFree(d_enc8); hipFree(d_enc16);
    /* JPEG output: the same frame as a one-component baseline file through the four entry points — header on the host,
     * coefficients and scan on the device, the length word read back, header || scan || EOI written to argv[1] if given */
    {
        enum { QUALITY = 90, RI = 8 };
        uint8_t head[1024];
        size_t head_len = 0, coef_bytes = 0, scratch_bytes = 0, max_scan = 0;
        CHECK_HHSR(hhsr_jpeg_header(H, W, 1, QUALITY, RI, head, sizeof head, &head_len));
        CHECK_HHSR(hhsr_jpeg_workspace(H, W, 1, RI, &coef_bytes, &scratch_bytes, &max_scan));
        if (head_len < 300 || head[0] != 0xFF || head[1] != 0xD8 || head[2] != 0xFF || head[3] != 0xE0 ||
            head[head_len - 1] != 0 || head[head_len - 2] != 63) { fprintf(stderr, "jpeg header is malformed\n"); return 1; }
        const size_t capacity = (size_t)2 * H * W; /* the first guess of the Python layer; max_scan always suffices */
        int16_t* d_coef;
        void* d_scratch;
        uint8_t* d_scan;
        uint64_t *d_len, len = 0;
        CHECK_HIP(hipMalloc((void**)&d_coef, coef_bytes));
        CHECK_HIP(hipMalloc(&d_scratch, scratch_bytes));
        CHECK_HIP(hipMalloc((void**)&d_scan, capacity));
        CHECK_HIP(hipMalloc((void**)&d_len, sizeof len));
        CHECK_HHSR(hhsr_jpeg_dct(d_norm, H, W, 1, 1, QUALITY, d_coef, coef_bytes, NULL));
        CHECK_HHSR(hhsr_jpeg_entropy(d_coef, H, W, 1, RI, d_scratch, scratch_bytes, d_scan, capacity, d_len, NULL));
        CHECK_HIP(hipMemcpy(&len, d_len, sizeof len, hipMemcpyDeviceToHost));
        if (len == 0 || len > capacity || capacity > max_scan) { fprintf(stderr, "jpeg scan of %llu bytes, capacity %zu, bound %zu\n", (unsigned long long)len, capacity, max_scan); return 1; }
        uint8_t* scan = (uint8_t*)malloc((size_t)len + 2);
        CHECK_HIP(hipMemcpy(scan, d_scan, (size_t)len, hipMemcpyDeviceToHost));
        scan[len] = 0xFF; scan[len + 1] = 0xD9; /* EOI */
        if (argc > 1) {
            FILE* f = fopen(argv[1], "wb");
            if (!f || fwrite(head, 1, head_len, f) != head_len || fwrite(scan, 1, (size_t)len + 2, f) != (size_t)len + 2 || fclose(f)) {
                fprintf(stderr, "cannot write %s\n", argv[1]);
                return 1;
            }
        }
        printf("jpeg: %zu header bytes + %llu scan bytes (capacity %zu, bound %zu) + EOI%s%s\n", head_len, (unsigned long long)len,
               capacity, max_scan, argc > 1 ? " -> " : "", argc > 1 ? argv[1] : "");
        free(scan);
        if (hhsr_jpeg_dct(d_norm, H, W, 1, 1, 0, d_coef, coef_bytes, NULL) == 0) return 1; /* quality 0: refused */
        hipFree(d_coef); hipFree(d_scratch); hipFree(d_scan); hipFree(d_len);
    }
    /* argument errors come back as codes + messages, never as exceptions */
    if (hhsr_gauss_decimate(d_norm, H, W, W, d_lvl, w2, 3, taps, NT, NULL) == 0) return 1;
    printf("rejected factor 3: %s\n", hhsr_last_error());
    free(lvl);
    hipFree(d_counts); hipFree(d_norm); hipFree(d_lvl);
    return worst < 1e-5 ? 0 : 1;
}
