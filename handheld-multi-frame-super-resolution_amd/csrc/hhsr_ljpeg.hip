// DNG input: lossless JPEG tiles and strips decoded on the GPU (include/hhsr.h, "DNG input: lossless JPEG").
// The stream rules live in hhsr_ljpeg_core.h, shared with hhsr_ljpeg_decode_host; this unit holds the C ABI and the launch.
#include "hhsr_common.h"
#include "hhsr_ljpeg_core.h"

namespace {

constexpr int LJ_BLOCK = 64;  // one wave per workgroup: the segments spread over as many CUs as there are waves

struct LjArgs {
    const uint8_t* blob;
    uint64_t blob_bytes;
    const hhsr_ljpeg_segment* segs;
    int n_segs;
    const hhsr_ljpeg_table* tables;
    int n_tables;
    uint16_t* workspace;
    uint64_t workspace_elems;
    uint16_t* out;
    int n_frames, H, W;
    int64_t row_elems, frame_elems;
    int32_t* status;
    int lanes;  // segments per workgroup (1..LJ_BLOCK): its first `lanes` lanes take one each
};

// One lane per segment.  Huffman decoding is serial within a stream, so a lane walks its own stream and the lanes of a wave
// diverge where their codes differ in length class; the host spreads the segments thinly (lanes < 64) while there are fewer
// segments than the chip has lanes to give, because a wave issues at the same rate for 1 active lane as for 64.
// LDS: the n_tables <= HHSR_LJPEG_LDS_TABLES decode tables, staged once per workgroup as dwords; else read from global.
template <bool LDS>
__global__ void __launch_bounds__(LJ_BLOCK) k_ljpeg_decode(LjArgs a) {
    __shared__ hhsr_ljpeg_table sm[LDS ? HHSR_LJPEG_LDS_TABLES : 1];
    if (LDS) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tables);
        uint32_t* dst = reinterpret_cast<uint32_t*>(sm);
        const int n = a.n_tables * (int)(sizeof(hhsr_ljpeg_table) / 4);
        for (int i = threadIdx.x; i < n; i += LJ_BLOCK) dst[i] = src[i];
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * a.lanes + threadIdx.x;
    if ((int)threadIdx.x >= a.lanes || i >= a.n_segs) return;
    const hhsr_ljpeg_segment s = a.segs[i];
    const hhsr_ljpeg_table* tabs;
    if constexpr (LDS)
        tabs = sm;
    else
        tabs = a.tables;
    a.status[i] = hhsr_lj::decode_segment(a.blob, a.blob_bytes, s, tabs, a.n_tables, a.workspace,
                                          a.workspace_elems, a.out, a.n_frames, a.H, a.W, a.row_elems, a.frame_elems);
}

int lj_check(const char* fn, const uint8_t* blob, size_t blob_bytes, const hhsr_ljpeg_segment* segs, int n_segs,
             const hhsr_ljpeg_table* tables, int n_tables, uint16_t* workspace, uint16_t* out, int n_frames, int H, int W,
             int64_t row_elems, int64_t frame_elems, int32_t* status) {
#define LJ_ARG(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            hhsr_set_error("%s: invalid argument: %s", fn, #cond);    \
            return -1;                                                \
        }                                                             \
    } while (0)
    LJ_ARG(blob && segs && tables && workspace && out && status);
    LJ_ARG(n_segs > 0 && n_tables > 0 && n_frames > 0 && H > 0 && W > 0);
    LJ_ARG(((uintptr_t)blob & 3) == 0 && (blob_bytes & 3) == 0);
    LJ_ARG(((uintptr_t)workspace & 1) == 0 && ((uintptr_t)out & 1) == 0);
    LJ_ARG(((uintptr_t)segs & 7) == 0 && ((uintptr_t)tables & 3) == 0 && ((uintptr_t)status & 3) == 0);
    LJ_ARG(row_elems >= W);
    LJ_ARG(frame_elems / H >= row_elems);  // frame_elems >= H row_elems, without the product
#undef LJ_ARG
    return 0;
}

}  // namespace

extern "C" int hhsr_ljpeg_parse(const uint8_t* stream_bytes, size_t n_bytes, hhsr_ljpeg_info* info) {
    HHSR_ARG(stream_bytes != nullptr && info != nullptr);
    const char* why = hhsr_lj::parse(stream_bytes, n_bytes, info);
    if (why) {
        hhsr_set_error("hhsr_ljpeg_parse: invalid argument: %s", why);
        return -1;
    }
    return 0;
}

extern "C" int hhsr_ljpeg_tables(const uint8_t* bits, const uint8_t* values, int n, hhsr_ljpeg_table* out) {
    HHSR_ARG(bits != nullptr && values != nullptr && out != nullptr && n > 0);
    HHSR_ARG(((uintptr_t)out & 3) == 0);
    for (int i = 0; i < n; ++i) {
        const bool prefix_code_with_values_up_to_16 = hhsr_lj::build_table(bits + 16 * (size_t)i, values + 17 * (size_t)i, out + i);
        HHSR_ARG(prefix_code_with_values_up_to_16);
    }
    return 0;
}

extern "C" int hhsr_ljpeg_workspace(hhsr_ljpeg_segment* segs, int n, size_t* bytes) {
    HHSR_ARG(segs != nullptr && bytes != nullptr && n > 0);
    const bool lines_fit = hhsr_lj::assign_workspace(segs, n, bytes);
    HHSR_ARG(lines_fit /* X in 1..65535, Nf in 1..4, fewer than 2^32 elements in all */);
    return 0;
}

extern "C" int hhsr_ljpeg_decode(const uint8_t* blob, size_t blob_bytes, const hhsr_ljpeg_segment* segs, int n_segs,
                                 const hhsr_ljpeg_table* tables, int n_tables, uint16_t* workspace, size_t workspace_bytes,
                                 uint16_t* out, int n_frames, int H, int W, int64_t row_elems, int64_t frame_elems,
                                 int32_t* status, void* stream) {
    if (int rc = lj_check(__func__, blob, blob_bytes, segs, n_segs, tables, n_tables, workspace, out, n_frames, H, W,
                          row_elems, frame_elems, status))
        return rc;
    // 2048 waves fill the chip's 1024 SIMDs twice: below that, fewer segments per wave instead of idle CUs
    int lanes = (n_segs + 2047) / 2048;
    lanes = lanes < 1 ? 1 : (lanes > LJ_BLOCK ? LJ_BLOCK : lanes);
    const LjArgs a{blob, (uint64_t)blob_bytes, segs, n_segs, tables, n_tables, workspace,
                   (uint64_t)(workspace_bytes / sizeof(uint16_t)), out, n_frames, H, W, row_elems, frame_elems, status, lanes};
    const dim3 grid((unsigned)((n_segs + lanes - 1) / lanes)), block(LJ_BLOCK);
    if (n_tables <= HHSR_LJPEG_LDS_TABLES)
        hipLaunchKernelGGL(k_ljpeg_decode<true>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_ljpeg_decode<false>, grid, block, 0, (hipStream_t)stream, a);
    HHSR_LAUNCHED();
}

extern "C" int hhsr_ljpeg_decode_host(const uint8_t* blob, size_t blob_bytes, const hhsr_ljpeg_segment* segs, int n_segs,
                                      const hhsr_ljpeg_table* tables, int n_tables, uint16_t* workspace,
                                      size_t workspace_bytes, uint16_t* out, int n_frames, int H, int W, int64_t row_elems,
                                      int64_t frame_elems, int32_t* status) {
    if (int rc = lj_check(__func__, blob, blob_bytes, segs, n_segs, tables, n_tables, workspace, out, n_frames, H, W,
                          row_elems, frame_elems, status))
        return rc;
    for (int i = 0; i < n_segs; ++i)
        status[i] = hhsr_lj::decode_segment(blob, (uint64_t)blob_bytes, segs[i], tables, n_tables, workspace,
                                            (uint64_t)(workspace_bytes / sizeof(uint16_t)), out, n_frames, H, W, row_elems,
                                            frame_elems);
    return 0;
}
