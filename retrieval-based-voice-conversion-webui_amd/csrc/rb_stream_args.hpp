// Kernel arguments of k_rb_stream (rb_stream_kernels.hpp): plain data, shared with the host interface (rb_stream.hpp), whose plans hold them.
#pragma once

namespace rvcmi {

constexpr int RS_MAXND = 3;

struct RbStreamJob {
    const float* src;
    float* dst;
    const void* w1[RS_MAXND];
    const void* w2[RS_MAXND];
    const float* b1[RS_MAXND];
    const float* b2[RS_MAXND];
    long ct1, ct2;       // packed elements per 32-channel output tile
    int k, k_p;          // real / padded taps
    int dil[RS_MAXND];
    int blk0;            // first blockIdx.x of this job
    int nstrips;
    int strip_len;       // output rows per strip
    int sx_off[RS_MAXND];  // LDS row offset of pair m's X history inside the side area
    int sh_off[RS_MAXND];  // ... and of its H history
};
struct RbStreamArgs {
    RbStreamJob job[3];
    int njobs;
    int B;          // utterances; the grid is (sum of nstrips) * B blocks
    int L;
    const int* lens;  // ragged batch (mfma_conv.hpp item_rows)
    int lmul;
    long bstride;
    int side_rows;  // rows of the side area (max over jobs)
    int flags;      // bit 2 (4) = lean K loop instantiation; bit 3 (8) = the dst streams are fp16 (pack4_h, mfma_conv.hpp), same
                    // element layout; bit 4 (16) = the src stream is fp16 (KL = 2 only); bit 5 (32) = a strip's first step skips its
                    // pipeline-fill column tiles (rs_fill_tile); bit 6 (64) = the K loops run on v_mfma_f32_16x16x32 (SH = 16)
    unsigned long long* ts;  // dev only (RVCMI_RS_STAMPS=1): per-wave cycle sums per phase, [block][wave][16]
};

}  // namespace rvcmi
