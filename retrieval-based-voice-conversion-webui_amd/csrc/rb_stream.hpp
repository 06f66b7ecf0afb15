// Host interface of the streaming fused ResBlock kernel (rb_stream_kernels.hpp); implemented in rb_stream.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "rb_stream_args.hpp"

namespace rvcmi {

struct RbStreamDesc {  // one resblock (ND = 3: all its pairs) or one pair level of it (ND = 1)
    const float* src;
    float* dst;
    const void* w1[3];
    const void* w2[3];
    const float* b1[3];
    const float* b2[3];
    long ct1, ct2;
    int k, k_p;
    int dil[3];
    int y_half;  // (jobs[0] decides for the launch) dst streams are fp16; only k_rb_stream itself honours it
    int x_half;  // (jobs[0]) src is an fp16 stream (round 5: X0 of the streaming stage, option X0_F16); needs the lean-K-loop instantiation
    const int* lens;  // (jobs[0]) ragged batch: item b holds lens[b] * lmul rows (mfma_conv.hpp item_rows); nullptr = all L
    int lmul;
};

// Sets the per-device kernel attributes (dynamic LDS > 64 KB) of every instantiation; called from rvcmi_nsf_create.
void rb_stream_prepare();
// Channel counts / fusion depths the kernel is instantiated for.
bool rb_stream_supported(int operand, int C, int nd);
// Option keys read from `opt` (dev / tests): RS_SMALL (0 = the larger time tiles), RS_KL (2 = k_rb_stream with the lean K loop
// kconv), RS_C0 (planning constant), RS_STAMPS (print phase stamps; syncs), RS_FILL (0 = a strip's first step computes its pipeline-fill
// column tiles too, as every later step does; unset / 1 = skips them), RS_MFMA (16 / 32: the MFMA shape of the lean-K-loop instantiations, v_mfma_f32_16x16x32 / 32x32x16; the shape a launch
// takes is RbStreamPlan::mfma()).
inline void rb_stream_load_env(Options& opt) { opt.load_env({"RS_SMALL", "RS_KL", "RS_C0", "RS_STAMPS", "RS_FILL", "RS_MFMA"}); }
// One launch of the kernel, planned: strips for `B` utterances of `L` rows, ONE grid covering all `njobs` resblocks.
struct RbStreamPlan {
    bool ok;            // false: refused (halo too large for the tile, fp16 input rows outside the kernel form that reads them, or strips too short
                        // for the persistent walk to pay and `force` not set); nothing below is meaningful then
    RbStreamArgs args;  // per job k, nstrips and strip_len; flags
    int operand, C, nd;
    int NJ, NCO;        // the instantiation's class: steps of 32 * NJ rows, blocks of NCO waves
    int nblocks;        // per utterance: the grid is nblocks * B blocks
    size_t lds_bytes;   // dynamic LDS of the launch
    bool lean() const { return (args.flags & 4) != 0; }       // the lean K loop (KL = 2)
    bool y_half() const { return (args.flags & 8) != 0; }
    bool x_half() const { return (args.flags & 16) != 0; }
    bool fill_skip() const { return (args.flags & 32) != 0; }
    int mfma() const { return (args.flags & 64) ? 16 : 32; }  // MFMA shape of the K loops
};
RbStreamPlan rb_stream_plan(int operand, int C, int nd, const RbStreamDesc* jobs, int njobs, int L, int B, long bstride, bool force, const Options& opt);
// Launches exactly that (accepted) plan.  `opt` is read for RS_STAMPS only.
void rb_stream_run(const RbStreamPlan& p, hipStream_t st, const Options& opt);

}  // namespace rvcmi
