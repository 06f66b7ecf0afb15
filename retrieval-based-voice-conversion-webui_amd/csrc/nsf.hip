// Host side of the generator: weight preparation (stands in for rvc/synthesizer.py:10-28 for
// `net_g.dec`), workspace, and the launch sequence of NSFGenerator.forward (rvc/layers/nsf.py:145-191)
// / Generator.forward (rvc/layers/generators.py:70-98).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>

#include "common.hpp"
#include "nsf_source_kernels.hpp"
#include "conv_kernels.hpp"
#include "post_kernels.hpp"
#include "rb_pair_kernels.hpp"
#include "ups_kernels.hpp"
#include "rb_full_kernels.hpp"
#include "conv_pack.hpp"
#include "rb_stream.hpp"

namespace rvcmi {

struct Geom {
    int MI, NJ, WCO, TT;
};
// Block/wave tiling per output-channel count (see k_conv_mfma): waves split output channels first
// (each wave streams its OWN weight slice), time second.
static Geom conv_geom(int cout) {
    Geom g;
    g.NJ = 4;
    if (cout >= 256) { g.MI = 2; g.WCO = 4; }
    else if (cout >= 128) { g.MI = 2; g.WCO = 2; }
    else if (cout >= 64) { g.MI = 2; g.WCO = 1; }
    else { g.MI = 1; g.WCO = 1; }
    g.TT = (4 / g.WCO) * g.NJ * 32;
    return g;
}

struct Stage {
    int cin, cout, u, k, pad;
    ConvLayer up;
    // noise conv (nsf.py:103-115)
    int nk = 0, ns = 1, npad = 0;
    DevBuf noise_w, noise_b;
    ConvLayer nz;          // the same noise conv as a 2-tap MFMA conv over frames of `ns` samples (when ns % 8 == 0)
    bool nz_mfma = false;
    DevBuf nz_k1_w;        // ... or, for windows of <= 16 samples, as ONE extra k-step inside k_ups
    bool nz_k1 = false;
    // resblocks[j].pair[m] = {conv1, conv2}
    std::vector<std::vector<std::pair<ConvLayer, ConvLayer>>> rb;
};

}  // namespace rvcmi

using namespace rvcmi;

struct rvcmi_nsf {
    rvcmi_nsf_config cfg;
    int device = 0;
    int max_B = 0, max_T = 0;
    int upp = 1;
    int C0 = 0;
    ConvLayer pre;
    DevBuf cond_w, cond_b;
    float lin_w = 1.f, lin_b = 0.f;
    std::vector<Stage> stages;
    DevBuf post_w;
    int c_last = 0;
    // workspace
    size_t S = 0;  // elements per activation buffer
    // P: conv_pre output.  X0: ups(+noise) output = input of the stage's resblocks.  Ya[j]/Yb[j]: ping-pong
    // fp32 streams of resblock j (its final output is one of them; the consumer sums the nk of them).
    DevBuf P, X0, Ya[RVCMI_MAX_RB], Yb[RVCMI_MAX_RB], H, NZ, har, har2, x2, phase, condv, dbg;
    size_t ws_bytes = 0;
    Profiler prof;
    // what the last forward planned, per stage it reached (rvcmi_nsf_last_plan)
    rvcmi_nsf_stage_plan last_plan[RVCMI_MAX_UPS];
    int n_plan = 0;
    // dev / test options (common.hpp Options): RB_STREAM (absent = auto, 1 = streaming resblock kernels whenever supported, 0 = never),
    // NO_RB_SPLIT, Y_F16, X0_F16, X0_F16_NOSTREAM, POST_DMA, POST_DBG, RBF_PAD_TAP, RBF32_TALL, DBG (timing-ablation bit mask: results are WRONG when
    // non-zero) and
    // the rb_stream keys (rb_stream.hpp).  Read from RVCMI_<KEY> once, in rvcmi_nsf_create.
    rvcmi::Options opt;
};

namespace rvcmi {


static void set_lds_limits();
constexpr int RB_KG = 4;  // k-steps per weight-prefetch group inside the fused resblock kernel
constexpr int RB256_NJ = 4;  // (96-row tiles, 2 blocks per CU, measured the same 0.33 ms at B=1; 128 rows reuse weights better)
static int rb_rows(int C) { return C == 256 ? 32 * RB256_NJ : RB_ROWS; }
// Resblock stages of at most this many rows (B x L) at C = 256 run conv by conv, split over output channels (run_conv_jobs): a
// realtime chunk's first stage is 310 rows = 9 fused pair tiles, each pulling 2.9 MB of weights through ONE CU (3 x 70 us).
constexpr int RB_SPLIT_MAX_ROWS = 1024;      // C = 256
constexpr int RB_SPLIT_MAX_ROWS_128 = 4096;  // C = 128 (a chunk's second stage: 3100 rows = 75 pair tiles of 3 x 40 us)

// Weights of upsampling stage i: ups[i], noise_convs[i] and its resblocks.
static void build_stage(Stage& s, const rvcmi_nsf_config* cfg, WeightTable& wm, int i) {
    const int op = cfg->operand, C0 = cfg->upsample_initial_channel;
    s.cin = C0 >> i;
    s.cout = C0 >> (i + 1);
    s.u = cfg->upsample_rates[i];
    s.k = cfg->upsample_kernel_sizes[i];
    s.pad = (s.k - s.u) / 2;
    if (s.u > 16) RVCMI_FAIL(RVCMI_ERR_INVALID, "upsample rate %d > 16 unsupported", s.u);
    if (s.cout < 4 || (s.cout & 3)) RVCMI_FAIL(RVCMI_ERR_INVALID, "stage %d has %d channels", i, s.cout);
    // The reference requires len(ups) == len(noise_convs): (L-1)*u - 2*pad + k == u*L  <=>  k - 2*pad == u
    if (s.k - 2 * s.pad != s.u) RVCMI_FAIL(RVCMI_ERR_INVALID, "stage %d: k-u must be even (k=%d,u=%d)", i, s.k, s.u);
    {  // ups[i]: ConvTranspose1d(cin, cout, k, u, padding=(k-u)//2)   nsf.py:92-102
        // out[q*u + r] = sum_j x[q + off_r - j] * W[:, :, cm_r + j*u],  c = r + pad, off_r = c / u, cm_r = c % u
        const float* w = wm.get("ups." + std::to_string(i) + ".weight", {s.cin, s.cout, s.k});
        const float* b = wm.get("ups." + std::to_string(i) + ".bias", {s.cout});
        int nt[16], off[16], cm[16];
        for (int r = 0; r < s.u; ++r) {
            const int c = r + s.pad;
            off[r] = c / s.u;
            cm[r] = c % s.u;
            nt[r] = (s.k - cm[r] + s.u - 1) / s.u;
        }
        const int cout = s.cout, k = s.k, u = s.u;
        std::vector<int> cmv(cm, cm + s.u);
        build_conv(s.up, s.cin, s.cout, s.u, nt, off, -1,
                   [=](int co, int ci, int p, int tap) { return w[((size_t)ci * cout + co) * k + cmv[p] + tap * u]; },
                   b, op);
    }
    if (cfg->use_f0) {  // noise_convs[i]   nsf.py:103-115
        int sf = 1;
        for (int j = i + 1; j < cfg->n_ups; ++j) sf *= cfg->upsample_rates[j];
        const bool last = i + 1 == cfg->n_ups;
        s.nk = last ? 1 : 2 * sf;
        s.ns = last ? 1 : sf;
        s.npad = last ? 0 : sf / 2;
        const float* w = wm.get("noise_convs." + std::to_string(i) + ".weight", {s.cout, 1, s.nk});
        const float* b = wm.get("noise_convs." + std::to_string(i) + ".bias", {s.cout});
        std::vector<float> wt((size_t)s.nk * s.cout);
        for (int co = 0; co < s.cout; ++co)
            for (int j = 0; j < s.nk; ++j) wt[(size_t)j * s.cout + co] = w[(size_t)co * s.nk + j];
        upload(s.noise_w, wt);
        upload(s.noise_b, b, s.cout * sizeof(float));
        if (op != RVCMI_OPERAND_F32 && !last && s.ns % 8 == 0 && s.ns <= 64) {
            const int cinp = s.ns <= 16 ? 16 : (s.ns <= 32 ? 32 : 64);
            int nt = 2, off = 0;
            const int ns = s.ns, nkk = s.nk;
            build_conv(s.nz, cinp, s.cout, 1, &nt, &off, 1,
                       [=](int co, int ci, int, int tap) { return ci < ns ? w[(size_t)co * nkk + tap * ns + ci] : 0.f; }, b, op);
            s.nz_mfma = true;
        } else if (op != RVCMI_OPERAND_F32 && s.nk >= 2 && s.nk <= 16 && s.ns % 2 == 0) {
            const int ctiles = (s.cout + 31) / 32;
            std::vector<uint16_t> pk((size_t)ctiles * 512, 0);
            for (int ct = 0; ct < ctiles; ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int co = ct * 32 + (lane & 31), kk = 8 * (lane >> 5) + e;
                        if (co < s.cout && kk < s.nk) {
                            const float v = w[(size_t)co * s.nk + kk];
                            pk[(size_t)ct * 512 + lane * 8 + e] = op == RVCMI_OPERAND_BF16 ? f32_to_bf16(v) : f32_to_f16(v);
                        }
                    }
            upload(s.nz_k1_w, pk);
            s.nz_k1 = true;
        }
    }
    s.rb.resize(cfg->n_resblock_kernels);
    for (int j = 0; j < cfg->n_resblock_kernels; ++j) {  // ResBlock1   residuals.py:19-58
        const int n = i * cfg->n_resblock_kernels + j;
        const int k = cfg->resblock_kernel_sizes[j];
        const int nd = cfg->n_dilations[j];
        if (nd < 1 || nd > RVCMI_MAX_DIL || !(k & 1)) RVCMI_FAIL(RVCMI_ERR_INVALID, "bad resblock %d", j);
        s.rb[j].resize(nd);
        for (int m = 0; m < nd; ++m) {
            const int d = cfg->resblock_dilation_sizes[j][m];
            const std::string base = "resblocks." + std::to_string(n);
            const int C = s.cout;
            for (int which = 0; which < 2; ++which) {
                const std::string nm = base + (which ? ".convs2." : ".convs1.") + std::to_string(m);
                const float* w = wm.get(nm + ".weight", {C, C, k});
                const float* b = wm.get(nm + ".bias", {C});
                const int dil = which ? 1 : d;
                int nt = k, off = -((k * dil - dil) / 2);  // get_padding, rvc/layers/utils.py:14
                ConvLayer& L2 = which ? s.rb[j][m].second : s.rb[j][m].first;
                build_conv(L2, C, C, 1, &nt, &off, dil,
                           [=](int co, int ci, int, int tap) { return w[((size_t)co * C + ci) * k + tap]; }, b, op);
            }
        }
    }
}

static void nsf_create(const rvcmi_nsf_config* cfg, const rvcmi_tensor* weights, int n_weights, int device, int max_B,
                       int max_T, rvcmi_nsf** out) {
    if (!cfg || !out || (!weights && n_weights)) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
    if (cfg->n_ups < 1 || cfg->n_ups > RVCMI_MAX_UPS || cfg->n_resblock_kernels < 1 ||
        cfg->n_resblock_kernels > RVCMI_MAX_RB)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "bad stage counts");
    if (cfg->operand < 0 || cfg->operand > 2) RVCMI_FAIL(RVCMI_ERR_INVALID, "bad operand type %d", cfg->operand);
    if (max_B < 1 || max_T < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "max_B/max_T must be positive");
    HIP_CHECK(hipSetDevice(device));
    set_lds_limits();
    rb_stream_prepare();

    std::unique_ptr<rvcmi_nsf> h(new rvcmi_nsf());
    h->opt.load_env({"RB_STREAM", "NO_RB_SPLIT", "POST_DMA", "POST_DBG", "RBF_PAD_TAP", "RBF32_TALL", "DBG", "Y_F16", "X0_F16", "X0_F16_NOSTREAM"});
    rb_stream_load_env(h->opt);
    h->cfg = *cfg;
    h->device = device;
    h->max_B = max_B;
    h->max_T = max_T;
    const int op = cfg->operand;
    WeightTable wm(weights, n_weights, "nsf_create");

    const int C0 = cfg->upsample_initial_channel, inter = cfg->inter_channels;
    h->C0 = C0;
    {  // conv_pre: Conv1d(inter, C0, 7, padding=3)   nsf.py:84-86
        const float* w = wm.get("conv_pre.weight", {C0, inter, 7});
        const float* b = wm.get("conv_pre.bias", {C0});
        int nt = 7, off = -3;
        build_conv(h->pre, inter, C0, 1, &nt, &off, 1,
                   [=](int co, int ci, int, int tap) { return w[((size_t)co * inter + ci) * 7 + tap]; }, b, op);
    }
    if (cfg->gin_channels) {  // cond: Conv1d(gin, C0, 1)   nsf.py:129-130
        const float* w = wm.get("cond.weight", {C0, cfg->gin_channels, 1});
        const float* b = wm.get("cond.bias", {C0});
        upload(h->cond_w, w, (size_t)C0 * cfg->gin_channels * sizeof(float));
        upload(h->cond_b, b, C0 * sizeof(float));
    }
    if (cfg->use_f0) {  // m_source.l_linear: Linear(1,1)   nsf.py:51
        h->lin_w = wm.get("m_source.l_linear.weight", {1, 1})[0];
        h->lin_b = wm.get("m_source.l_linear.bias", {1})[0];
    }
    int upp = 1;
    for (int i = 0; i < cfg->n_ups; ++i) upp *= cfg->upsample_rates[i];
    h->upp = upp;

    h->stages.resize(cfg->n_ups);
    size_t S = (size_t)max_T * C0;
    long L = max_T;
    for (int i = 0; i < cfg->n_ups; ++i) {
        build_stage(h->stages[i], cfg, wm, i);
        L *= h->stages[i].u;
        S = std::max(S, (size_t)L * h->stages[i].cout);
    }
    h->c_last = C0 >> cfg->n_ups;
    {  // conv_post: Conv1d(ch, 1, 7, padding=3, bias=False)   nsf.py:126
        const float* w = wm.get("conv_post.weight", {1, h->c_last, 7});
        std::vector<float> wt((size_t)7 * h->c_last);
        for (int c = 0; c < h->c_last; ++c)
            for (int j = 0; j < 7; ++j) wt[(size_t)j * h->c_last + c] = w[(size_t)c * 7 + j];
        upload(h->post_w, wt);
    }
    if (h->c_last & 3) RVCMI_FAIL(RVCMI_ERR_INVALID, "last stage channel count %d", h->c_last);

    // workspace
    if (cfg->n_resblock_kernels > 3) RVCMI_FAIL(RVCMI_ERR_INVALID, "more than 3 resblock kernels per stage is unsupported");
    h->S = S * (size_t)max_B;
    const size_t fb = h->S * sizeof(float);
    h->P.alloc((size_t)max_B * max_T * C0 * sizeof(float));
    h->X0.alloc(fb);
    for (int j = 0; j < cfg->n_resblock_kernels; ++j) {
        h->Ya[j].alloc(fb);
        h->Yb[j].alloc(fb);
    }
    if (op == RVCMI_OPERAND_F32) h->H.alloc(fb);
    else h->H.alloc((size_t)3 * std::max(RB_SPLIT_MAX_ROWS * 256, RB_SPLIT_MAX_ROWS_128 * 128) * 2);  // conv1 outputs of the output-channel-split resblock path (tiny launches)
    {
        size_t nz = 0;
        long Ls = max_T;
        for (int i = 0; i < cfg->n_ups; ++i) {
            Ls *= cfg->upsample_rates[i];
            if (h->stages[i].nz_mfma) nz = std::max(nz, (size_t)Ls * h->stages[i].cout);
        }
        if (nz) h->NZ.alloc(nz * max_B * sizeof(float));
    }
    const size_t hb = (size_t)max_B * max_T * upp * sizeof(float);
    h->har.alloc(hb);
    h->har2.alloc(hb);
    h->x2.alloc((size_t)max_B * inter * max_T * sizeof(float));
    h->phase.alloc((size_t)max_B * max_T * sizeof(float));
    h->condv.alloc((size_t)max_B * C0 * sizeof(float));
    HIP_CHECK(hipMemset(h->condv.p, 0, h->condv.bytes));
    h->ws_bytes = (size_t)(1 + 2 * cfg->n_resblock_kernels + (op == RVCMI_OPERAND_F32 ? 1 : 0)) * fb + h->P.bytes + 2 * hb + h->x2.bytes + h->phase.bytes + h->condv.bytes;
    *out = h.release();
}

// ---- launches -----------------------------------------------------------------------------------

template <typename OpT, int CIN, int MI, int NJ, int WCO>
static void launch_inst(const ConvArgs& a, int B, hipStream_t st) {
    using TL = Tile<CIN>;
    constexpr int TT = (4 / WCO) * NJ * 32;
    const int co_blocks = (a.cout + 32 * MI * WCO - 1) / (32 * MI * WCO);
    dim3 grid((a.Lq + TT - 1) / TT, co_blocks * a.nphase, B);
    const size_t smem = (size_t)a.tile_rows * TL::STRIDE;
    if (smem > 160 * 1024) RVCMI_FAIL(RVCMI_ERR_INVALID, "LDS tile too large: %zu bytes (cin %d)", smem, CIN);
    hipLaunchKernelGGL((k_conv_mfma<OpT, CIN, MI, NJ, WCO>), grid, dim3(256), smem, st, a);
}

template <typename OpT, int CIN, int MI, int NJ, int WCO>
static void set_lds_inst() {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_conv_mfma<OpT, CIN, MI, NJ, WCO>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
}

#define RVCMI_FOR_EACH_CIN(X, OpT, MI, NJ, WCO) \
    X(OpT, 16, MI, NJ, WCO)                     \
    X(OpT, 32, MI, NJ, WCO)                     \
    X(OpT, 64, MI, NJ, WCO)                     \
    X(OpT, 128, MI, NJ, WCO)                    \
    X(OpT, 192, MI, NJ, WCO)                    \
    X(OpT, 256, MI, NJ, WCO)                    \
    X(OpT, 512, MI, NJ, WCO)

template <typename OpT, int MI, int NJ, int WCO>
static void launch_by_cin(const ConvArgs& a, int B, hipStream_t st) {
    switch (a.cin) {
#define X(OpT_, CIN_, MI_, NJ_, WCO_) \
    case CIN_:                        \
        return launch_inst<OpT_, CIN_, MI_, NJ_, WCO_>(a, B, st);
        RVCMI_FOR_EACH_CIN(X, OpT, MI, NJ, WCO)
#undef X
        default:
            RVCMI_FAIL(RVCMI_ERR_INVALID, "unsupported C_in %d for the MFMA path", a.cin);
    }
}

template <typename OpT>
static void launch_conv_mfma(const ConvArgs& a, int nj, int B, hipStream_t st) {
    const Geom g = conv_geom(a.cout);
    if (g.MI == 2 && g.WCO == 4 && nj == 1) return launch_by_cin<OpT, 2, 1, 4>(a, B, st);
    if (g.MI == 2 && g.WCO == 4) return launch_by_cin<OpT, 2, 4, 4>(a, B, st);
    if (g.MI == 2 && g.WCO == 2) return launch_by_cin<OpT, 2, 4, 2>(a, B, st);
    if (g.MI == 2 && g.WCO == 1) return launch_by_cin<OpT, 2, 4, 1>(a, B, st);
    return launch_by_cin<OpT, 1, 4, 1>(a, B, st);
}

template <typename OpT>
static void set_lds_all() {
#define X(OpT_, CIN_, MI_, NJ_, WCO_) set_lds_inst<OpT_, CIN_, MI_, NJ_, WCO_>();
    RVCMI_FOR_EACH_CIN(X, OpT, 2, 4, 4)
    RVCMI_FOR_EACH_CIN(X, OpT, 2, 1, 4)
    RVCMI_FOR_EACH_CIN(X, OpT, 2, 4, 2)
    RVCMI_FOR_EACH_CIN(X, OpT, 2, 4, 1)
    RVCMI_FOR_EACH_CIN(X, OpT, 1, 4, 1)
#undef X
}
template <typename OpT>
static void set_lds_rb();
template <typename OpT>
static void set_lds_ups();
static void set_lds_rbf();
static void set_lds_limits() {
    set_lds_all<__bf16>();
    set_lds_all<_Float16>();
    set_lds_rb<__bf16>();
    set_lds_rb<_Float16>();
    set_lds_ups<__bf16>();
    set_lds_ups<_Float16>();
    set_lds_rbf();
}


template <typename OpT, int C, int MI, int NW, int KG, int NJ = RB_ROWS / 32, int NWT = 1, int OCC = 2>
static void launch_rb_inst(const RbPairArgs& ra, int tiles, int nj, int B, int rows, hipStream_t st) {
    const size_t smem = (size_t)rows * Tile<C>::STRIDE + 2 * 32 * MI * NW * 4 + NW * NWT * 64;  // tile + the two bias vectors + dev stamps
    if (smem > 160 * 1024) RVCMI_FAIL(RVCMI_ERR_INVALID, "resblock LDS tile too large (%zu B)", smem);
    hipLaunchKernelGGL((k_rb_pair<OpT, C, MI, NW, KG, NJ, NWT, OCC>), dim3(tiles, nj, B), dim3(64 * NW * NWT), smem, st, ra);
}
template <typename OpT>
static void launch_rb_pair_t(int C, const RbPairArgs& ra, int tiles, int nj, int B, int rows, hipStream_t st) {
    switch (C) {
        case 256: return launch_rb_inst<OpT, 256, 2, 4, RB_KG, RB256_NJ>(ra, tiles, nj, B, rows, st);
        case 128: return launch_rb_inst<OpT, 128, 2, 2, RB_KG>(ra, tiles, nj, B, rows, st);
        case 64: return launch_rb_inst<OpT, 64, 2, 1, RB_KG>(ra, tiles, nj, B, rows, st);
        case 32: return launch_rb_inst<OpT, 32, 1, 1, RB_KG>(ra, tiles, nj, B, rows, st);
        case 16: return launch_rb_inst<OpT, 16, 1, 1, RB_KG>(ra, tiles, nj, B, rows, st);
        default: RVCMI_FAIL(RVCMI_ERR_INVALID, "unsupported resblock channel count %d", C);
    }
}
static void launch_rb_pair(int op, int C, const RbPairArgs& ra, int tiles, int nj, int B, int rows, hipStream_t st) {
    if (op == RVCMI_OPERAND_BF16) launch_rb_pair_t<__bf16>(C, ra, tiles, nj, B, rows, st);
    else launch_rb_pair_t<_Float16>(C, ra, tiles, nj, B, rows, st);
}
template <typename OpT>
static void set_lds_rb() {
#define RB_ATTR(C_, MI_, NW_)                                                                                   \
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rb_pair<OpT, C_, MI_, NW_, RB_KG>),           \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_rb_pair<OpT, 256, 2, 4, RB_KG, RB256_NJ>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    RB_ATTR(128, 2, 2) RB_ATTR(64, 2, 1) RB_ATTR(32, 1, 1) RB_ATTR(16, 1, 1)
#undef RB_ATTR
}

template <typename OpT, int CIN, int MI, int WV>
static void launch_ups_inst(UpsArgs a, int nj, int B, hipStream_t st) {
    const int TQ = 32 * nj * (4 / WV);
    size_t smem = (size_t)a.tile_rows * Tile<CIN>::STRIDE + (a.nz_k1 ? (size_t)(TQ * a.u * a.ns + 16) * 2 : 0);
    // a.bias_off: [2][cout] fp32 LDS copy of bias / bn.  Reserved FIRST so that both bounds below see it (appended after
    // the checks, a 52 KB block became 54 KB -- two resident blocks instead of three -- and a tile near 160 KB would have failed at launch);
    // dropped where it would break the 160 KB limit
    if (a.bias_off && a.cout % 4 == 0 && (smem + 15) / 16 * 16 + (size_t)2 * a.cout * 4 <= 160 * 1024) {
        smem = (smem + 15) / 16 * 16;
        a.bias_off = (int)smem;
        smem += (size_t)2 * a.cout * 4;
    } else {
        a.bias_off = 0;
    }
    if (smem > 160 * 1024) RVCMI_FAIL(RVCMI_ERR_INVALID, "upsampler LDS tile too large (%zu B)", smem);
    const int per_block = WV * a.vpw;
    dim3 grid((a.Lin + TQ - 1) / TQ, (a.nvt + per_block - 1) / per_block, B);
    // row-wise output through an LDS tile when the block owns whole rows (all phases and channels) and the tile keeps the block small
    // enough for three per CU (everything counted: operand tile, har copy, bias copy, output tile); (cout * esz) must be whole 16-byte chunks
    {
        const int esz = a.out_half ? 2 : 4;
        const size_t ot = (size_t)TQ * a.u * ((size_t)a.cout * esz + 16);
        smem = (smem + 15) / 16 * 16;
        if (a.out_tr && grid.y == 1 && (a.cout * esz) % 16 == 0 && smem + ot <= 52 * 1024) {
            a.out_tr_off = (int)smem;
            smem += ot;
        } else {
            a.out_tr = 0;
        }
    }
    // ... else, for one-tile waves writing fp16 (stage 1 of v2/48k: 10 phases x 128 channels, the block's output tile would be 87 KB): wave-private
    // transposition tiles, so that the stores are whole 128-byte lines (a.out_tw_off)
    if (a.out_tw_off && !a.out_tr && a.out_half && nj == 1 && MI == 2 && a.cout % 64 == 0) {
        smem = (smem + 15) / 16 * 16;
        a.out_tw_off = (int)smem;
        smem += (size_t)4 * 32 * (MI * 64 + 16);
    } else {
        a.out_tw_off = 0;
    }
    if (nj == 4) hipLaunchKernelGGL((k_ups<OpT, CIN, MI, WV, 4>), grid, dim3(256), smem, st, a);
    else if (nj == 2) hipLaunchKernelGGL((k_ups<OpT, CIN, MI, WV, 2>), grid, dim3(256), smem, st, a);
    else hipLaunchKernelGGL((k_ups<OpT, CIN, MI, WV, 1>), grid, dim3(256), smem, st, a);
}
#define RVCMI_UPS_CASES(X, OpT) \
    X(OpT, 512, 2) X(OpT, 256, 2) X(OpT, 128, 2) X(OpT, 64, 1) X(OpT, 32, 1)
template <typename OpT>
static void launch_ups_t(const UpsArgs& a, int wv, int nj, int B, hipStream_t st) {
#define X(OpT_, CIN_, MI_)                                                        \
    if (a.cin == CIN_) {                                                          \
        if (wv == 4) return launch_ups_inst<OpT_, CIN_, MI_, 4>(a, nj, B, st);    \
        if (wv == 2) return launch_ups_inst<OpT_, CIN_, MI_, 2>(a, nj, B, st);    \
        return launch_ups_inst<OpT_, CIN_, MI_, 1>(a, nj, B, st);                 \
    }
    RVCMI_UPS_CASES(X, OpT)
#undef X
    RVCMI_FAIL(RVCMI_ERR_INVALID, "unsupported upsampler C_in %d", a.cin);
}
template <typename OpT>
static void set_lds_ups() {
#define Y(OpT_, CIN_, MI_, WV_, NJ_)                                                                                    \
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ups<OpT_, CIN_, MI_, WV_, NJ_>),                      \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#define X(OpT_, CIN_, MI_)                                                                                              \
    Y(OpT_, CIN_, MI_, 4, 4) Y(OpT_, CIN_, MI_, 4, 2) Y(OpT_, CIN_, MI_, 4, 1) Y(OpT_, CIN_, MI_, 2, 4) Y(OpT_, CIN_, MI_, 2, 2)   \
    Y(OpT_, CIN_, MI_, 2, 1) Y(OpT_, CIN_, MI_, 1, 4) Y(OpT_, CIN_, MI_, 1, 2) Y(OpT_, CIN_, MI_, 1, 1)
    RVCMI_UPS_CASES(X, OpT)
#undef Y
#undef X
}

// ---- fully fused resblock (C <= 64) ----------------------------------------------------------------
// One launch of k_rb_full for the whole stage; the tile classes it is instantiated for are the rows of RBF_CLASSES below.
// `ra` == nullptr: only set the > 64 KB dynamic-LDS attribute of the instantiation (set_lds_limits).
template <typename OpT, int C, int MI, int NJ, int NB, int OCC, int NWV>
static void launch_rbf(size_t smem, const RbFullArgs* ra, int tiles, int nj, int B, hipStream_t st) {
    auto kern = &k_rb_full<OpT, C, MI, NJ, /*KG*/ 4, NB, OCC, NWV>;
    if (!ra) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        return;
    }
    hipLaunchKernelGGL(kern, dim3(tiles, nj, B), dim3(64 * NWV), smem, st, *ra);
}
struct RbFullClass {
    int C, rows, waves;      // rows = waves x 32 NJ: what a block computes; a resblock keeps rows - 2 halo of them
    int MI, NJ, NB, OCC;     // the template parameters: NB = weight-prefetch depth (register buffers), OCC = blocks per CU
    size_t lds_bytes;        // X | H operand tiles + bias vectors + the bytes reserved for the dev phase stamps
    void (*launch[2])(size_t, const RbFullArgs*, int, int, int, hipStream_t);  // bf16, fp16 operands
};
#define RBF_CLASS(C_, MI_, NJ_, NB_, OCC_, NWV_, STAMP_B_)                                                                     \
    {C_, NWV_ * 32 * NJ_, NWV_, MI_, NJ_, NB_, OCC_,                                                                           \
     (size_t)(2 * (NWV_ * 32 * NJ_) + 2 * RBF_G + 2 * RBF_G2) * Tile<C_>::STRIDE + 3 * 2 * 32 * MI_ * 4 + STAMP_B_,            \
     {&launch_rbf<__bf16, C_, MI_, NJ_, NB_, OCC_, NWV_>, &launch_rbf<_Float16, C_, MI_, NJ_, NB_, OCC_, NWV_>}}
static constexpr RbFullClass RBF_CLASSES[] = {
    // The default classes.  C = 64, 512 rows: 8 waves (2 per SIMD) x 64 rows: the co-resident wave hides the K loop's issue overhead, and the larger
    // tile wastes less on overlap-save than 384 rows (x + h accumulators: 64 + 64 registers per wave; 256 registers per wave, a 2-deep ring fits)
    RBF_CLASS(64, 2, 2, 2, 2, 8, 512),
    // C <= 32, 384 rows: keeps the two operand tiles at 68 KB and the kernel under 256 registers => 2 blocks per CU, so one block's load /
    // publish / store phases overlap the other's MFMA phases (worth more than the extra overlap-save waste of a 512-row tile of four waves,
    // which is what it was measured against)
    RBF_CLASS(32, 1, 3, 3, 2, 4, 512),
    RBF_CLASS(16, 1, 3, 3, 2, 4, 512),
    // 256 rows, for a launch of a few tiles.  C = 64 (a realtime chunk's 6200 rows = 44 tiles of 512 rows on 256 CUs, the launch as long as ONE
    // k = 11 tile: 50 us): four waves -- 107 blocks, each half as long; two accumulator sets of 64 registers + a 3-deep ring: no spills.
    RBF_CLASS(64, 2, 2, 3, 1, 4, 512),
    // C = 32, two blocks per CU: a chunk's 12 400 rows are 122 tiles of 384 rows, 214 of 256
    RBF_CLASS(32, 1, 2, 3, 2, 4, 512),
    // C = 32, 768 rows, for a launch of many tiles: the same eight waves per CU as ONE block (X | H: 129 KB of LDS), the same work and registers
    // per wave, 648 / 696 / 744 kept rows of 768 instead of 264 / 312 / 360 of 384
    RBF_CLASS(32, 1, 3, 3, 1, 8, 1024),
};
#undef RBF_CLASS
constexpr int RBF_SMALL_ROWS = 256, RBF_TALL_ROWS = 768;
static int rbf_default_rows(int C) { return C == 64 ? 512 : 384; }
static const RbFullClass* rbf_class(int C, int rows) {
    for (const RbFullClass& c : RBF_CLASSES)
        if (c.C == C && c.rows == rows) return &c;
    RVCMI_FAIL(RVCMI_ERR_INVALID, "fused resblock: no %d-row tile class for channel count %d", rows, C);
}
static void set_lds_rbf() {
    for (const RbFullClass& c : RBF_CLASSES)
        for (auto launch : c.launch) launch(c.lds_bytes, nullptr, 0, 0, 0, nullptr);
}

// A three-way option: 0 = never, 1 = always, absent (or anything else) = 2, the planner decides.
static int tri_mode(const rvcmi_nsf* h, const char* key) {
    const int v = h->opt.has(key) ? h->opt.geti(key, 2) : 2;
    return v == 0 || v == 1 ? v : 2;
}
// option RBF32_TALL: absent = auto (plan_stage), 1 = the 768-row class at C = 32 always, 0 = never.
static int rbf32_tall_mode(const rvcmi_nsf* h) { return tri_mode(h, "RBF32_TALL"); }
// option RB_STREAM: absent = auto (streaming kernel when the strips are long enough), 1 = always when supported, 0 = never.
static int rb_stream_mode(const rvcmi_nsf* h) { return tri_mode(h, "RB_STREAM"); }

// Option Y_F16 (default 1): the whole-ResBlock kernels (k_rb_stream ND = 3, k_rb_full) write their output streams Ya[j] as fp16
// and the next stage's k_ups / k_post read them as such (mfma_conv.hpp pack4_h).  0 = fp32 streams (round 3).
static bool y_f16(const rvcmi_nsf* h) {
    return h->cfg.operand != RVCMI_OPERAND_F32 && h->opt.geti("Y_F16", 1) != 0;
}

static void run_conv(rvcmi_nsf* h, const ConvLayer& L, ConvArgs a, int B, const char* name, hipStream_t st) {
    if (!a.cf_stride) a.cf_stride = a.Lin;
    a.cin = L.cin;
    a.cout = L.cout;
    a.bias = L.bias.as<float>();
    a.dstep = L.dstep;
    a.nphase = L.nphase;
    const int op = h->cfg.operand;
    int jsum = 0;
    for (int p = 0; p < L.nphase; ++p) {
        a.ph_in_off[p] = L.in_off[p];
        a.ph_ntaps[p] = L.ntaps[p];
        a.ph_w_off[p] = op == RVCMI_OPERAND_F32 ? L.f32_off[p] : L.pack_off[p];
        jsum += L.ntaps[p];
    }
    a.in_off = L.in_off[0];
    const double flops = L.flops_per_pos * (double)a.Lq * B;
    const size_t esz = op == RVCMI_OPERAND_F32 ? 4 : 2;
    double bytes = (double)B * a.Lin * L.cin * (a.in_mode == IN_OP_RAW ? esz : 4) +
                   (double)B * a.Lq * L.nphase * L.cout * (a.out_mode == OUT_ACT ? esz : 4) * (a.accumulate ? 2 : 1) +
                   (a.res ? (double)B * a.Lq * L.nphase * L.cout * 4 : 0) + (double)jsum * L.cin * L.cout * esz;
    if (op == RVCMI_OPERAND_F32) {
        a.w = L.w_f32.p;
        a.ntaps = L.ntaps[0];
        a.roff = 0;
        a.tile_rows = 0;
        const size_t n = (size_t)a.Lq * a.cout;
        dim3 grid((unsigned)((n + 255) / 256), L.nphase, B);
        h->prof.launch(name, flops, bytes, st, [&] { hipLaunchKernelGGL(k_conv_f32, grid, dim3(256), 0, st, a); });
    } else {
        Geom g = conv_geom(L.cout);
        // a launch of a few dozen 128-row tiles (conv_pre of one clip: 20 blocks) is latency-bound on one tile's K loop:
        // 32-row tiles give 4x the blocks and a quarter of the per-block work
        int nj = 4;
        if (g.MI == 2 && g.WCO == 4 && (long)B * ((a.Lq + g.TT - 1) / g.TT) * ((L.cout + 255) / 256) * L.nphase < 128) {
            nj = 1;
            g.TT = 32;
        }
        a.w = L.w_pack.p;
        a.w_ct_stride = L.ct_stride;
        a.ntaps = L.ntaps_p;
        const int span = (L.ntaps_p - 1) * std::abs(L.dstep);
        a.roff = L.dstep < 0 ? span : 0;
        // (conv_pre of a realtime chunk through the K-split blocks was measured: 18 -> 14 us -- and removed: a second summation order for
        //  calls of at most 128 frames breaks "a ragged batch item is bit-equal to its separate call" for no pinned option)
        a.tile_rows = g.TT + span;
        h->prof.launch(name, flops, bytes, st, [&] {
            if (op == RVCMI_OPERAND_BF16) launch_conv_mfma<__bf16>(a, nj, B, st);
            else launch_conv_mfma<_Float16>(a, nj, B, st);
        });
    }
    HIP_CHECK(hipGetLastError());
}

// Up to three independent convs of the same shape class (C_in = C_out = 256 or 128) in ONE launch of k_conv_ks_jobs
// (conv_kernels.hpp conv_ks_body): 32 NJ rows x 32 channels per block, the four waves split the taps.
constexpr int conv_ks_nj(int C) { return C == 256 ? 1 : 3; }  // rows per block / 32 (C = 128: 96-row tiles = 396 blocks for a chunk's 3100 rows)
template <typename OpT, int C>
static void launch_conv_ks_jobs(const ConvJobs& js, int Lq, int B, size_t smem, hipStream_t st) {
    static std::atomic<unsigned long long> attr_done{0};
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    constexpr int NJ = conv_ks_nj(C);
    auto kern = &k_conv_ks_jobs<OpT, C, 1, NJ>;
    if (!(attr_done.load() & (1ull << (dev & 63)))) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_done.fetch_or(1ull << (dev & 63));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((Lq + 32 * NJ - 1) / (32 * NJ)), C / 32, (unsigned)(B * js.njobs)), dim3(256), smem, st, js);
}
// Realtime chunk, ABAB, against blocks that run all the taps of 128 rows: C = 256 (310 rows, 32-row tiles = 240 blocks) six launches
// 134 -> 107 us; C = 128 (3100 rows) 113 -> 107 us with 96-row tiles (396 blocks) -- with 32-row tiles it LOST (155 us: 1164 blocks that
// each stage 82 rows for 32 outputs).
static void run_conv_jobs(rvcmi_nsf* h, const ConvLayer* const* Ls, const ConvArgs* as, int nj, int B, const char* name, hipStream_t st) {
    ConvJobs js;
    memset(&js, 0, sizeof(js));
    js.njobs = nj;
    double flops = 0, bytes = 0;
    size_t smem = 0;
    for (int j = 0; j < nj; ++j) {
        const ConvLayer& L = *Ls[j];
        ConvArgs a = as[j];
        if ((L.cin != 256 && L.cin != 128) || L.cout != L.cin || L.cin != Ls[0]->cin || L.nphase != 1 || L.dstep < 0)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "run_conv_jobs: unsupported layer");
        a.cin = L.cin;
        a.cout = L.cout;
        a.bias = L.bias.as<float>();
        a.dstep = L.dstep;
        a.nphase = 1;
        a.in_off = L.in_off[0];
        a.w = L.w_pack.p;
        a.w_ct_stride = L.ct_stride;
        a.ntaps = L.ntaps_p;
        a.roff = 0;
        const int ksr = 32 * conv_ks_nj(L.cin);
        a.tile_rows = ksr + (L.ntaps_p - 1) * L.dstep;
        smem = std::max(smem, (size_t)a.tile_rows * (2 * L.cin + 16) + (size_t)3 * (ksr / 32) * 16 * 64 * 4);  // (+ the partial sums of 3 waves)
        flops += L.flops_per_pos * (double)a.Lq * B;
        bytes += (double)B * a.Lq * L.cin * (a.in_mode == IN_OP_RAW ? 2 : 4) + (double)B * a.Lq * L.cin * (a.out_mode == OUT_ACT ? 2 : 4) +
                 (a.res ? (double)B * a.Lq * L.cin * 4 : 0) + (double)L.ntaps[0] * L.cin * L.cin * 2;
        js.job[j] = a;
    }
    const bool c256 = Ls[0]->cin == 256;
    h->prof.launch(name, flops, bytes, st, [&] {
        if (h->cfg.operand == RVCMI_OPERAND_BF16) {
            if (c256) launch_conv_ks_jobs<__bf16, 256>(js, as[0].Lq, B, smem, st);
            else launch_conv_ks_jobs<__bf16, 128>(js, as[0].Lq, B, smem, st);
        } else {
            if (c256) launch_conv_ks_jobs<_Float16, 256>(js, as[0].Lq, B, smem, st);
            else launch_conv_ks_jobs<_Float16, 128>(js, as[0].Lq, B, smem, st);
        }
    });
    HIP_CHECK(hipGetLastError());
}

// option DBG: timing-ablation bit mask forwarded to the kernels (results are WRONG when non-zero; bench/dev only).
static int dbg_flags(const rvcmi_nsf* h) { return h->opt.geti("DBG", 0); }

static ConvArgs base_args() {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.slope_in = 0.1f;
    a.div_in = 1.f;
    a.slope_out = 0.1f;
    a.out_mul = 1;
    a.nphase = 1;
    return a;
}

struct TapRequest {
    const char* what = nullptr;
    float* out_host = nullptr;
    size_t capacity = 0;
    int64_t* shape = nullptr;
    bool done = false;
};

static void copy_tap_cl(rvcmi_nsf* h, const float* src_cl, int B, int L, int C, TapRequest* tr, hipStream_t st) {
    const size_t n = (size_t)B * L * C;
    if (n > tr->capacity) RVCMI_FAIL(RVCMI_ERR_NOMEM, "tap needs %zu floats, capacity %zu", n, tr->capacity);
    if (h->dbg.bytes < n * 4) h->dbg.alloc(n * 4);
    dim3 grid((unsigned)(((size_t)L * C + 255) / 256), B);
    hipLaunchKernelGGL(k_cl_to_cf, grid, dim3(256), 0, st, src_cl, h->dbg.as<float>(), L, C);
    HIP_CHECK(hipMemcpyAsync(tr->out_host, h->dbg.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    tr->shape[0] = B;
    tr->shape[1] = C;
    tr->shape[2] = L;
    tr->done = true;
}

// dev only (DBG & 32, RVCMI_DEV_STAMPS builds): a zeroed buffer of `n` per-wave phase stamps for the fused resblock kernels ...
static unsigned long long* stamp_buffer(rvcmi_nsf* h, size_t n, hipStream_t st) {
    if (h->dbg.bytes < n * 8) h->dbg.alloc(n * 8);
    HIP_CHECK(hipMemsetAsync(h->dbg.p, 0, n * 8, st));
    return h->dbg.as<unsigned long long>();
}
// ... and its readback: the cycles between consecutive stamps of batch item 0's blocks, averaged per job (resblock kernel size).
// Stamps [job][tile][wave][nst]; a wave that wrote no first stamp, or a phase it never reached, counts nothing.
template <typename Args>
static void print_stamps(rvcmi_nsf* h, const char* nm, const Args& ra, int njobs, int max_tiles, int nwv, int nst, size_t nblk,
                         hipStream_t st) {
    HIP_CHECK(hipStreamSynchronize(st));
    std::vector<unsigned long long> ts(nblk * nwv * nst);
    HIP_CHECK(hipMemcpy(ts.data(), h->dbg.p, ts.size() * 8, hipMemcpyDeviceToHost));
    for (int oj = 0; oj < njobs; ++oj) {
        double sum[16] = {0};
        long cnt = 0;
        for (int t = 0; t < ra.job[oj].ntiles; ++t)
            for (int w = 0; w < nwv; ++w) {
                const unsigned long long* p = &ts[(((size_t)oj * max_tiles + t) * nwv + w) * nst];
                if (!p[0]) continue;
                for (int i = 1; i < nst; ++i) sum[i] += p[i] ? (double)(p[i] - p[i - 1]) : 0.0;
                ++cnt;
            }
        fprintf(stderr, "[rvcmi ts] %s k=%d tiles=%d:", nm, ra.job[oj].k, ra.job[oj].ntiles);
        for (int i = 1; i < nst; ++i) fprintf(stderr, " %.0f", cnt ? sum[i] / cnt : 0.0);
        fprintf(stderr, "\n");
    }
}

// ---- forward ------------------------------------------------------------------------------------

// What every step of one forward call shares.
struct Fwd {
    rvcmi_nsf* h;
    int op, B, Te;       // Te: frames after the realtime interpolation (n_res)
    const int* lens;     // ragged batch: valid frames per item (device [B]) or nullptr
    const int* nres;     // rvcmi_nsf_forward_nres: interpolation target per item (device [B], <= Te) or nullptr.  The excitation runs over all T
                         // input frames of every item whatever it says; behind the interpolation it is the layers' `lens`
    const float* har;    // excitation [B][Te * upp] (use_f0)
    hipStream_t st;
    TapRequest* tr;
    rvcmi_nsf_stage_plan* rec;  // the running stage's record in the handle (rvcmi_nsf_last_plan)
    bool want(const char* w) const { return tr && strcmp(tr->what, w) == 0; }
};

// The running activation ((y[0] + y[1]) + y[2]) / div, [B][L][C] rows (nsf.py:177-186); stage 0 reads conv_pre's P alone.
struct Act {
    const float* y[3];
    bool half;  // y[] are fp16 streams (written by k_rb_stream ND = 3 / k_rb_full under option Y_F16)
    bool raw;   // y[0] holds the activated operands already (conv_pre on the MFMA path)
    float div;
    long L;
    int C;
    int lm;     // rows per frame (ragged batches: item rows = lens[b] * lm)
};

using RbLevels = std::vector<std::pair<ConvLayer, ConvLayer>>;  // one resblock: {conv1, conv2} per dilation

// How a stage's resblocks run, in order of precedence (plan_stage):
//   F32_CHAIN  fp32 operands: conv by conv
//   SPLIT      a handful of rows (realtime chunk): conv1 / conv2 of all resblocks as output-channel-split launches per pair level
//   STREAM     whole resblocks on the streaming kernel (rb_stream_kernels.hpp): persistent blocks walk strips of the time axis
//   FULL       whole resblocks fused, x resident in registers (C <= 64): ONE launch for the stage   residuals.py:68-85
//   PAIR       one launch per pair level (k_rb_pair, or at C = 256 the streaming kernel with ND = 1 where its planner takes it)
enum class RbPath { F32_CHAIN = RVCMI_RB_F32_CHAIN, SPLIT = RVCMI_RB_SPLIT, STREAM = RVCMI_RB_STREAM, FULL = RVCMI_RB_FULL, PAIR = RVCMI_RB_PAIR };
struct StagePlan {
    RbPath path;
    bool x0_half;     // the upsampler writes X0 as fp16
    bool stage_half;  // the resblocks write their output streams as fp16
    const RbFullClass* full;  // FULL: the tile class (a row of RBF_CLASSES)
    RbStreamPlan stream;      // STREAM: the launch, planned, with the flops and bytes the profiler books for it
    double flops, bytes;
};

static float* ydst(rvcmi_nsf* h, size_t j, size_t m) { return (m & 1) ? h->Yb[j].as<float>() : h->Ya[j].as<float>(); }

static size_t max_levels(const Stage& s) {
    size_t n = 0;
    for (const RbLevels& rb : s.rb) n = std::max(n, rb.size());
    return n;
}

// The stage's resblocks, heaviest kernel size first (the long blocks are dispatched first).
static void rb_order(const Stage& s, int* order) {
    const int nk = (int)s.rb.size();
    for (int j = 0; j < nk; ++j) order[j] = j;
    std::sort(order, order + nk, [&](int a, int b) { return s.rb[a][0].first.ntaps[0] > s.rb[b][0].first.ntaps[0]; });
}

// One-sided halo of a whole resblock in the fused kernel.
static int rbf_halo(const RbLevels& rb) {
    int dsum = 0;
    for (const auto& pr : rb) dsum += pr.first.dstep;
    return (rb[0].first.ntaps[0] - 1) / 2 * (dsum + (int)rb.size());
}

// Job descriptor (RbStreamDesc, RbFullJob) of pair levels [m0, m0 + nd) of one resblock; adds their flops and weight bytes over B x L rows.
template <typename D>
static void fill_rb_job(D& d, const RbLevels& rb, int m0, int nd, long L, int B, int C, double& flops, double& bytes) {
    d.k = rb[m0].first.ntaps[0];
    d.k_p = rb[m0].first.ntaps_p;
    d.ct1 = rb[m0].first.ct_stride;
    d.ct2 = rb[m0].second.ct_stride;
    for (int m = 0; m < nd; ++m) {
        const ConvLayer& c1 = rb[m0 + m].first;
        const ConvLayer& c2 = rb[m0 + m].second;
        d.w1[m] = c1.w_pack.p;
        d.w2[m] = c2.w_pack.p;
        d.b1[m] = c1.bias.as<float>();
        d.b2[m] = c2.bias.as<float>();
        d.dil[m] = c1.dstep;
        flops += (c1.flops_per_pos + c2.flops_per_pos) * (double)L * B;
        bytes += 2.0 * d.k * C * C * 2;
    }
}

// Whole resblocks of a stage as jobs of the streaming kernel (ND = 3): X0 -> Ya[j], heaviest first.
static void stream_jobs(const Fwd& f, const Stage& s, long L, int lm, bool xhalf, bool yhalf, RbStreamDesc* sd, double& flops,
                        double& bytes) {
    rvcmi_nsf* h = f.h;
    const int C = s.cout;
    int order[RVCMI_MAX_RB];
    rb_order(s, order);
    for (size_t oj = 0; oj < s.rb.size(); ++oj) {
        const int j = order[oj];
        RbStreamDesc& d = sd[oj];
        memset(&d, 0, sizeof(d));
        d.src = h->X0.as<float>();
        d.dst = h->Ya[j].as<float>();
        d.y_half = yhalf ? 1 : 0;
        d.x_half = xhalf ? 1 : 0;
        d.lens = f.lens;
        d.lmul = lm;
        fill_rb_job(d, s.rb[j], 0, 3, L, f.B, C, flops, bytes);
        bytes += (double)f.B * L * C * ((yhalf ? 2 : 4) + (xhalf ? 2 : 4));
    }
}

// Everything that decides how stage `s` (L rows per item, lm rows per frame) runs, decided once, before anything of it is launched:
// the upsampler's X0 dtype must match the resblock path that reads it.
static StagePlan plan_stage(const Fwd& f, const Stage& s, long L, int lm) {
    rvcmi_nsf* h = f.h;
    const int op = f.op, C = s.cout, nk = (int)s.rb.size();
    const bool yh = y_f16(h);
    // Option X0_F16 (default 1, only together with Y_F16): X0 -- read once per resblock -- is stored as fp16 where its consumer reads
    // fp16 rows: k_rb_full (C <= 64: the two HBM-heaviest stages of every shipped config) and -- round 5, unless X0_F16_NOSTREAM -- the
    // streaming kernel with its coalesced step IO.  Unlike the Y streams this rounds the START of the fp32 residual stream (relative 2^-11
    // once per stage; the stream itself stays fp32 inside the kernels): +1.1e-4 RMS on the full-clip golden, measured on the oracle and
    // gated by the same 5e-4 test.  0 = fp32 X0.
    const bool x0h = yh && h->opt.geti("X0_F16", 1) != 0;
    StagePlan p{RbPath::PAIR};
    if (op == RVCMI_OPERAND_F32) {
        p.path = RbPath::F32_CHAIN;
        return p;
    }
    const long rows = (long)f.B * L;
    const int mode = rb_stream_mode(h);
    // (round 6, review item 4: the same conv-by-conv launches for a FULL-length stage 0 with 64-channel x 256-row blocks -- 684 blocks per launch,
    //  no halo recompute -- were built as a dev option, parity-green, and measured 0.61 ms against k_rb_pair<256>'s 0.284 ms; removed)
    if (((C == 256 && rows <= RB_SPLIT_MAX_ROWS) || (C == 128 && rows <= RB_SPLIT_MAX_ROWS_128)) && nk <= 3 && !h->opt.on("NO_RB_SPLIT") &&
        mode != 1) {
        p.path = RbPath::SPLIT;
        return p;
    }
    bool stream = mode != 0 && nk <= 3 && rb_stream_supported(op, C, 3);
    for (int j = 0; j < nk; ++j) stream = stream && s.rb[j].size() == 3;
    if (stream) {
        // the planner refuses short strips, and fp16 input rows outside the kernel form that reads them (option RS_KL)
        auto plans = [&](bool xhalf) {
            RbStreamDesc sd[3];
            p.flops = p.bytes = 0;
            stream_jobs(f, s, L, lm, xhalf, yh, sd, p.flops, p.bytes);
            p.stream = rb_stream_plan(op, C, 3, sd, nk, (int)L, f.B, L * C, mode == 1, h->opt);
            return p.stream.ok;
        };
        const bool xh = x0h && !h->opt.on("X0_F16_NOSTREAM") && plans(true);
        if (xh || plans(false)) {
            p.path = RbPath::STREAM;
            p.x0_half = xh;
            p.stage_half = yh;
            return p;
        }
    }
    if (C <= 64 && max_levels(s) <= 3) {
        const int R0 = rbf_default_rows(C);
        p = {RbPath::FULL, x0h, yh, rbf_class(C, R0)};
        // (C = 64) short launches take 256-row tiles: at 512 rows they would be fewer blocks than half the CUs (halo of the k = 11
        // resblock: 120 rows either way -- the small tiles keep 136 of 256 rows)
        if (C == 64 || C == 32) {
            long blocks512 = 0, blocks768 = 0;
            bool fits768 = true;
            for (int j = 0; j < nk; ++j) {
                const int HL = rbf_halo(s.rb[j]);
                blocks512 += (L + (R0 - 2 * HL) - 1) / (R0 - 2 * HL) * f.B;
                if (RBF_SMALL_ROWS - 2 * HL < RBF_SMALL_ROWS / 4) blocks512 = 1 << 30;  // (halo too large for the small tile)
                blocks768 += (L + (RBF_TALL_ROWS - 2 * HL) - 1) / (RBF_TALL_ROWS - 2 * HL) * f.B;
                fits768 = fits768 && RBF_TALL_ROWS - 2 * HL >= RBF_TALL_ROWS / 4;
            }
            const bool small = blocks512 < num_cus() / 2 * (C == 64 ? 1 : 2);
            // (C = 32) long launches take 768-row tiles, one block of eight waves per CU: a quarter of the rows of a 384-row tile is halo,
            // 3 to 16 % of a 768-row one.  From four blocks per CU on, so that the tail of the launch (blocks twice as long) stays short.
            const int tall = C == 32 && fits768 ? rbf32_tall_mode(h) : 0;
            if (tall == 1 || (tall == 2 && !small && blocks768 >= 4L * num_cus())) p.full = rbf_class(C, RBF_TALL_ROWS);
            else if (small) p.full = rbf_class(C, RBF_SMALL_ROWS);
        }
    }
    return p;
}

// ---- excitation: har[B][Te*upp]                                           nsf.py:152-159
// Returns true when the "har" tap has been served (the forward ends there).
static bool excitation(Fwd& f, int T, const float* f0, const float* noise) {
    rvcmi_nsf* h = f.h;
    const rvcmi_nsf_config& c = h->cfg;
    const int B = f.B, Te = f.Te, upp = h->upp;
    hipStream_t st = f.st;
    const int* lens = f.nres ? nullptr : f.lens;  // (per-item n_res: every item's source covers its T input frames, nsf.py:152-154)
    h->prof.launch("phase_scan", 0, (double)B * T * 8, st, [&] {
        hipLaunchKernelGGL(k_phase_scan, dim3(B), dim3(256), 0, st, f0, h->phase.as<float>(), T, (float)c.sr, (float)upp, lens);
    });
    const size_t total = (size_t)B * T * upp;
    h->prof.launch("sine_source", 0, (double)total * (noise ? 8 : 4), st, [&] {
        hipLaunchKernelGGL(k_sine_source, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, f0,
                           h->phase.as<float>(), noise, h->har.as<float>(), T, upp, (float)c.sr, h->lin_w, h->lin_b, total);
    });
    f.har = h->har.as<float>();
    if (f.nres) {  // nsf.py:155-159 with a target per item; the row stride becomes Te * upp
        const size_t tot2 = (size_t)B * Te * upp;
        hipLaunchKernelGGL(k_interp_linear_ragged, dim3((unsigned)((tot2 + 255) / 256)), dim3(256), 0, st, f.har, h->har2.as<float>(), f.nres,
                           1, upp, T * upp, Te * upp, tot2);
        f.har = h->har2.as<float>();
    } else if (Te != T) {  // nsf.py:155-159
        const size_t tot2 = (size_t)B * Te * upp;
        hipLaunchKernelGGL(k_interp_linear, dim3((unsigned)((tot2 + 255) / 256)), dim3(256), 0, st, f.har,
                           h->har2.as<float>(), T * upp, Te * upp, tot2);
        f.har = h->har2.as<float>();
    }
    HIP_CHECK(hipGetLastError());
    if (!f.want("har")) return false;
    TapRequest* tr = f.tr;
    const size_t n = (size_t)B * Te * upp;
    if (n > tr->capacity) RVCMI_FAIL(RVCMI_ERR_NOMEM, "tap capacity");
    HIP_CHECK(hipMemcpyAsync(tr->out_host, f.har, n * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    tr->shape[0] = B; tr->shape[1] = 1; tr->shape[2] = (int64_t)Te * upp;
    tr->done = true;
    return true;
}

// ---- conv_pre + cond                                                       nsf.py:164-166
static Act conv_pre(const Fwd& f, const float* x, int T, const float* g) {
    rvcmi_nsf* h = f.h;
    const rvcmi_nsf_config& c = h->cfg;
    const int B = f.B, Te = f.Te, inter = c.inter_channels, C0 = h->C0;
    hipStream_t st = f.st;
    if (f.nres) {  // nsf.py:160-162 / generators.py:76-79 with a target per item
        const size_t tot = (size_t)B * inter * Te;
        hipLaunchKernelGGL(k_interp_linear_ragged, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x, h->x2.as<float>(), f.nres, inter, 1,
                           T, Te, tot);
        x = h->x2.as<float>();
    } else if (Te != T) {  // nsf.py:160-162 / generators.py:76-79
        const size_t tot = (size_t)B * inter * Te;
        hipLaunchKernelGGL(k_interp_linear, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, x, h->x2.as<float>(), T, Te, tot);
        x = h->x2.as<float>();
    }
    if (g && c.gin_channels) {
        hipLaunchKernelGGL(k_cond, dim3((C0 + 3) / 4, B), dim3(256), 0, st, g, h->cond_w.as<float>(),
                           h->cond_b.as<float>(), h->condv.as<float>(), c.gin_channels, C0);
    }
    float* P = h->P.as<float>();
    // round 6: on the MFMA path conv_pre writes the ACTIVATED OPERANDS to_op(lrelu(conv + bias + cond, 0.1)) -- the only thing stage 0's upsampler does
    // with P is to compute exactly that while staging (12 blocks per time tile each re-read and re-converted the fp32 rows) -- unless the fp32 "pre" tap is asked for
    const bool pre_op = f.op != RVCMI_OPERAND_F32 && !f.want("pre");
    ConvArgs a = base_args();
    a.in = x;
    a.in_bstride = (long)inter * Te;
    a.Lin = Te;
    a.in_mode = IN_F32_CF;
    a.Lq = Te;
    a.out_mode = pre_op ? OUT_ACT : OUT_F32;
    a.out = P;
    a.out_bstride = (long)Te * C0;
    a.out_C = C0;
    a.cb = (g && c.gin_channels) ? h->condv.as<float>() : nullptr;
    a.lens = f.lens;
    a.lmul_in = a.lmul_q = 1;
    run_conv(h, h->pre, a, B, "conv_pre", st);
    return Act{{P, nullptr, nullptr}, false, pre_op, 1.f, Te, C0, 1};
}

// ---- x = ups[i](leaky_relu(x, 0.1)) + noise_convs[i](har) -> X0 (L rows)    nsf.py:171-174
static void ups_f32(const Fwd& f, const Stage& s, const Act& x, long L, int lm) {
    rvcmi_nsf* h = f.h;
    const int C = s.cout, B = f.B;
    char nm[48];
    ConvArgs a = base_args();
    a.in = x.y[0];
    a.in_b = x.y[1];
    a.in_c = x.y[2];
    a.in_bstride = x.L * x.C;
    a.Lin = (int)x.L;
    a.in_mode = IN_F32_ACT;
    a.div_in = x.div;
    a.Lq = (int)x.L;
    a.out_mode = OUT_F32;
    a.out = h->X0.p;
    a.out_bstride = L * C;
    a.out_C = C;
    a.out_mul = s.u;
    a.lens = f.lens;
    a.lmul_in = a.lmul_q = x.lm;
    snprintf(nm, sizeof(nm), "ups_c%d", s.cin);
    run_conv(h, s.up, a, B, nm, f.st);
    if (h->cfg.use_f0) {
        const size_t n = (size_t)L * C;
        snprintf(nm, sizeof(nm), "noise_conv_c%d", C);
        h->prof.launch(nm, 2.0 * s.nk * n * B, (double)B * n * 8, f.st, [&] {
            hipLaunchKernelGGL(k_noise_add, dim3((unsigned)((n + 255) / 256), 1, B), dim3(256), 0, f.st, h->X0.as<float>(), f.har,
                               s.noise_w.as<float>(), s.noise_b.as<float>(), (int)L, C, f.Te * h->upp, s.nk, s.ns, s.npad, f.lens, lm, h->upp);
        });
    }
}

// ups + bias + noise conv in one MFMA kernel, X0 written once
static void ups_mfma(const Fwd& f, const Stage& s, const Act& x, const StagePlan& p, long L, int lm) {
    rvcmi_nsf* h = f.h;
    const int C = s.cout, B = f.B, upp = h->upp;
    const long Lin = x.L;
    const ConvLayer& U = s.up;
    char nm[48];
    UpsArgs ua;
    memset(&ua, 0, sizeof(ua));
    ua.dbg = dbg_flags(h);
    ua.bias_off = 1;    // LDS copy of bias / bn (the launcher turns it into the LDS offset where it fits)
    ua.in_a = x.y[0];
    ua.in_b = x.y[1];
    ua.in_c = x.y[2];
    ua.in_half = x.half ? 1 : 0;
    ua.in_raw = x.raw ? 1 : 0;
    ua.lens = f.lens;
    ua.lmul = x.lm;
    ua.lhmul = upp;
    ua.Lh_stride = f.Te * upp;
    ua.div = x.div;
    ua.Lin = (int)Lin;
    ua.cin = s.cin;
    ua.in_bstride = Lin * x.C;
    ua.w = U.w_pack.p;
    ua.ct_stride = U.ct_stride;
    int lo = 1 << 30, hi = -(1 << 30);
    for (int r = 0; r < s.u; ++r) {
        ua.ph_w_off[r] = U.pack_off[r];
        ua.ph_in_off[r] = U.in_off[r];
        lo = std::min(lo, U.in_off[r] - (U.ntaps_p - 1));
        hi = std::max(hi, U.in_off[r]);
    }
    ua.ntaps_p = U.ntaps_p;
    ua.u = s.u;
    ua.cout = C;
    ua.lo = lo;
    ua.bias = U.bias.as<float>();
    ua.out = h->X0.as<float>();
    ua.out_half = p.x0_half ? 1 : 0;
    ua.out_tr = 1;      // row-wise stores (the launcher clears it where the block does not own whole rows)
    ua.out_tw_off = 1;  // wave-private transposition tiles (the launcher turns it into the LDS offset where it applies)
    ua.out_bstride = L * C;
    if (h->cfg.use_f0 && s.nz_mfma) {  // noise_convs[i](har) as a 2-tap MFMA conv over frames -> NZ, added in k_ups' epilogue
        ConvArgs na = base_args();
        na.in = f.har;
        na.in_bstride = (long)f.Te * upp;
        na.Lin = f.Te * upp;
        na.in_mode = IN_HAR;
        na.hs = s.ns;
        na.hpad = s.npad;
        na.Lq = (int)L;
        na.out_mode = OUT_F32;
        na.out = h->NZ.p;
        na.out_bstride = L * C;
        na.out_C = C;
        na.lens = f.lens;
        na.lmul_in = upp;
        na.lmul_q = lm;
        snprintf(nm, sizeof(nm), "noise_mfma_c%d", C);
        run_conv(h, s.nz, na, B, nm, f.st);
        ua.addend = h->NZ.as<float>();
    } else if (h->cfg.use_f0) {
        ua.nz_k1 = s.nz_k1 ? 1 : 0;
        ua.wnz = s.nz_k1_w.p;
        ua.har = f.har;
        ua.Lh = f.Te * upp;
        ua.Wn = s.noise_w.as<float>();
        ua.bn = s.noise_b.as<float>();
        ua.nk = s.nk;
        ua.ns = s.ns;
        ua.npad = s.npad;
    }
    const int MIu = C >= 64 ? 2 : 1;
    ua.cog = (C + 32 * MIu - 1) / (32 * MIu);
    ua.nvt = s.u * ua.cog;
    const int wv = ua.nvt >= 4 ? 4 : (ua.nvt >= 2 ? 2 : 1);
    // time-tile height: blocks have equal duration, so a launch of ~1.1 x (resident blocks) runs two rounds for one
    // round of work; pick the largest tile that still gives >= 4 rounds of blocks (2 resident blocks per CU)
    // (measured at B = 1, same box, us: C_in 512: 52 / 36 / 37 for NJ 4 / 2 / 1; 256: 94 / 95 / 85; 128: 131 / 118 / 110;
    //  64 -> 32 channels: 98 / 102 / 150 -- with one 32-channel tile per wave, short tiles starve the MFMA of columns)
    int nj = 4;
    const long blocks4 = (long)((Lin + 128 * (4 / wv) - 1) / (128 * (4 / wv))) * B;
    if (blocks4 < 2048 && s.cin >= 128) nj = s.cin >= 512 ? 2 : 1;
    else if (blocks4 < 2048 && s.cin == 64) nj = 2;  // (us at B = 1 after the staging fix: 84 / 75 / 89 for NJ 4 / 2 / 1)
    // large grids (round 4, fp16 inputs + row-wise stores; us per clip at B = 16 for NJ 4 / 1 / 2, ABAB: C_in 128: 77 / 67 / 83,
    // 64: 70 / 73 / 55): the short tiles win there too -- they also keep the output tile inside the row-wise store's LDS budget
    else if (s.cin >= 512) nj = 2;   // (C_in 512: 22 vs 29 us for NJ 2 / 4; C_in 256 keeps NJ = 4: 52 vs 57)
    else if (s.cin == 128) nj = 1;
    else if (s.cin == 64) nj = 2;
    // (round 6: NJ 2 / 4 and vpw 1 / 2 for the C_in = 256 stage alone, 8 variants x 2, ABAB: 72-110 us against 60 -- every one loses)
    const int TQ = 32 * nj * (4 / wv);
    ua.tile_rows = TQ + (hi - lo);
    const long qtiles = (Lin + TQ - 1) / TQ;
    int vpw = (ua.nvt + wv - 1) / wv;  // everything in one block ...
    while (vpw > 1 && qtiles * B * ((ua.nvt + wv * vpw - 1) / (wv * vpw)) < 300) --vpw;  // ... unless the grid would starve
    ua.vpw = vpw;
    snprintf(nm, sizeof(nm), "ups_c%d", s.cin);
    const double flops = U.flops_per_pos * (double)Lin * B + 2.0 * s.nk * (double)L * C * B;
    const double bytes = (double)B * Lin * x.C * (x.half ? 2 : 4) * (x.y[1] ? (x.y[2] ? 3 : 2) : 1) + (double)B * L * C * (p.x0_half ? 2 : 4);
    h->prof.launch(nm, flops, bytes, f.st, [&] {
        if (f.op == RVCMI_OPERAND_BF16) launch_ups_t<__bf16>(ua, wv, nj, B, f.st);
        else launch_ups_t<_Float16>(ua, wv, nj, B, f.st);
    });
    HIP_CHECK(hipGetLastError());
}

// ---- resblocks[i*nk + j](x), j < nk: X0 -> src[j]                         nsf.py:175-185

// conv1 / conv2 of one resblock pair as two convs: hbuf = to_op(lrelu(conv1(lrelu(src)))), dst = src + conv2(hbuf)   residuals.py:73-82
static void rb_pair_args(const Fwd& f, long L, int C, int lm, const float* src, void* hbuf, float* dst, ConvArgs& a1, ConvArgs& a2) {
    a1 = base_args();
    a1.in = src;
    a1.in_mode = IN_F32_ACT;
    a1.out_mode = OUT_ACT;
    a1.out = hbuf;
    a2 = base_args();
    a2.in = hbuf;
    a2.in_mode = IN_OP_RAW;
    a2.out_mode = OUT_F32;
    a2.out = dst;
    a2.res = src;
    a2.res_bstride = L * C;
    for (ConvArgs* a : {&a1, &a2}) {
        a->in_bstride = L * C;
        a->Lin = (int)L;
        a->Lq = (int)L;
        a->lens = f.lens;
        a->lmul_in = a->lmul_q = lm;
        a->out_bstride = L * C;
        a->out_C = C;
    }
}

static void rb_f32_chain(const Fwd& f, const Stage& s, long L, int lm, const float** src) {
    rvcmi_nsf* h = f.h;
    char nm[48];
    snprintf(nm, sizeof(nm), "rb_c%d", s.cout);
    for (size_t j = 0; j < s.rb.size(); ++j)
        for (size_t m = 0; m < s.rb[j].size(); ++m) {
            float* dst = ydst(h, j, m);
            ConvArgs a1, a2;
            rb_pair_args(f, L, s.cout, lm, src[j], h->H.p, dst, a1, a2);
            run_conv(h, s.rb[j][m].first, a1, f.B, nm, f.st);
            run_conv(h, s.rb[j][m].second, a2, f.B, nm, f.st);
            src[j] = dst;
        }
}

static void rb_split(const Fwd& f, const Stage& s, long L, int lm, const float** src) {
    rvcmi_nsf* h = f.h;
    char nm[48];
    snprintf(nm, sizeof(nm), "rb_split_c%d", s.cout);
    for (size_t m = 0; m < max_levels(s); ++m) {
        const ConvLayer* L1[3];
        const ConvLayer* L2[3];
        ConvArgs a1[3], a2[3];
        int nj = 0;
        for (size_t j = 0; j < s.rb.size(); ++j) {
            if (m >= s.rb[j].size()) continue;
            float* dst = ydst(h, j, m);
            void* hbuf = (char*)h->H.p + (size_t)nj * (h->H.bytes / 3);
            rb_pair_args(f, L, s.cout, lm, src[j], hbuf, dst, a1[nj], a2[nj]);
            L1[nj] = &s.rb[j][m].first;
            L2[nj] = &s.rb[j][m].second;
            src[j] = dst;
            ++nj;
        }
        run_conv_jobs(h, L1, a1, nj, f.B, nm, f.st);
        run_conv_jobs(h, L2, a2, nj, f.B, nm, f.st);
    }
}

static void rb_stream(const Fwd& f, const Stage& s, const StagePlan& p, const float** src) {
    rvcmi_nsf* h = f.h;
    const int nk = (int)s.rb.size();
    char nm[48];
    snprintf(nm, sizeof(nm), "rb_stream_c%d", s.cout);
    h->prof.launch(nm, p.flops, p.bytes, f.st, [&] { rb_stream_run(p.stream, f.st, h->opt); });
    HIP_CHECK(hipGetLastError());
    rvcmi_nsf_stage_plan& r = *f.rec;
    r.n_rb = nk;
    r.stream_nj = p.stream.NJ;
    r.stream_mfma = p.stream.mfma();
    r.stream_fill_skip = p.stream.fill_skip();
    for (int j = 0; j < nk; ++j) {
        const RbStreamJob& J = p.stream.args.job[j];
        r.k[j] = J.k;
        r.tiles[j] = J.nstrips;
        r.strip_len[j] = J.strip_len;
        src[j] = h->Ya[j].as<float>();
    }
}

static void rb_full(const Fwd& f, const Stage& s, const StagePlan& p, long L, int lm, const float** src) {
    rvcmi_nsf* h = f.h;
    const int C = s.cout, nk = (int)s.rb.size(), B = f.B;
    char nm[48];
    snprintf(nm, sizeof(nm), "rb_full_c%d", C);
    RbFullArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.L = (int)L;
    ra.lens = f.lens;
    ra.lmul = lm;
    ra.bstride = L * C;
    ra.dbg = dbg_flags(h);
    ra.yh = p.stage_half ? 1 : 0;
    ra.xh = p.x0_half ? 1 : 0;
    ra.pad_tap = h->opt.geti("RBF_PAD_TAP", 0) != 0 ? 1 : 0;
    const int R = p.full->rows;
    rvcmi_nsf_stage_plan& r = *f.rec;
    r.tile_rows = R;
    r.tile_waves = p.full->waves;
    r.n_rb = nk;
    int order[RVCMI_MAX_RB];
    rb_order(s, order);
    int max_tiles = 0;
    double flops = 0, bytes = 0;
    for (int oj = 0; oj < nk; ++oj) {
        const int j = order[oj];
        RbFullJob& J = ra.job[oj];
        J.src = h->X0.as<float>();
        J.dst = h->Ya[j].as<float>();
        J.nd = (int)s.rb[j].size();
        fill_rb_job(J, s.rb[j], 0, J.nd, L, B, C, flops, bytes);
        for (int m = 0; m < J.nd; ++m)
            if (J.dil[m] * (J.k - 1) / 2 + J.dil[m] > RBF_G) RVCMI_FAIL(RVCMI_ERR_INVALID, "dilation too large for the fused resblock");
        J.HL = rbf_halo(s.rb[j]);
        J.tvalid = R - 2 * J.HL;
        if (J.tvalid < R / 4) RVCMI_FAIL(RVCMI_ERR_INVALID, "resblock halo too large for the fused kernel");
        J.ntiles = (int)((L + J.tvalid - 1) / J.tvalid);
        max_tiles = std::max(max_tiles, J.ntiles);
        r.k[oj] = J.k;
        r.tiles[oj] = J.ntiles;
        bytes += (double)B * L * C * ((p.stage_half ? 2 : 4) + (p.x0_half ? 2 : 4));
        src[j] = J.dst;
    }
    const size_t nblk = (size_t)max_tiles * nk * B;
    if (ra.dbg & 32) ra.ts = stamp_buffer(h, nblk * 8 * 16, f.st);
    h->prof.launch(nm, flops, bytes, f.st, [&] { p.full->launch[f.op == RVCMI_OPERAND_BF16 ? 0 : 1](p.full->lds_bytes, &ra, max_tiles, nk, B, f.st); });
    HIP_CHECK(hipGetLastError());
    if (ra.dbg & 32) print_stamps(h, nm, ra, nk, max_tiles, p.full->waves, 16, nblk, f.st);  // (waves per block: the stamp rows of a tile)
}

// One launch per pair level, heaviest kernel size first.  At C = 256 the streaming kernel (ND = 1) takes a level where its planner accepts it.
static void rb_pair(const Fwd& f, const Stage& s, long L, int lm, const float** src) {
    rvcmi_nsf* h = f.h;
    const int op = f.op, C = s.cout, nk = (int)s.rb.size(), B = f.B;
    const int mode = rb_stream_mode(h);
    char nm[48], nms[48];
    snprintf(nm, sizeof(nm), "rb_pair_c%d", C);
    snprintf(nms, sizeof(nms), "rb_stream1_c%d", C);
    int order[RVCMI_MAX_RB];
    rb_order(s, order);
    rvcmi_nsf_stage_plan& r = *f.rec;
    r.tile_rows = rb_rows(C);
    for (size_t m = 0; m < max_levels(s); ++m) {
        RbPairArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.lens = f.lens;
        ra.lmul = lm;
        ra.L = (int)L;
        ra.bstride = L * C;
        ra.dbg = dbg_flags(h);
        RbStreamDesc sd[RVCMI_MAX_RB];
        float* dsts[RVCMI_MAX_RB] = {nullptr};
        int nj = 0, max_tiles = 0, max_rows = 0;
        double flops = 0, bytes = 0;
        for (int oj = 0; oj < nk; ++oj) {
            const int j = order[oj];
            if (m >= s.rb[j].size()) continue;
            RbStreamDesc& d = sd[nj];
            memset(&d, 0, sizeof(d));
            d.src = src[j];
            d.dst = dsts[j] = ydst(h, j, m);
            d.lens = f.lens;
            d.lmul = lm;
            fill_rb_job(d, s.rb[j], (int)m, 1, L, B, C, flops, bytes);
            bytes += (double)B * L * C * 8;
            RbJob& J = ra.job[nj++];
            J.src = d.src; J.dst = d.dst; J.w1 = d.w1[0]; J.w2 = d.w2[0]; J.b1 = d.b1[0]; J.b2 = d.b2[0];
            J.ct1 = d.ct1; J.ct2 = d.ct2; J.k = d.k; J.k_p = d.k_p; J.dil = d.dil[0];
            J.tt2 = rb_rows(C) - (J.k - 1);
            J.ntiles = (int)((L + J.tt2 - 1) / J.tt2);
            max_tiles = std::max(max_tiles, J.ntiles);
            max_rows = std::max(max_rows, rb_rows(C) + (J.k_p - 1) * J.dil);
            if (m == 0) {  // (a resblock's tiles are those of its kernel size at every level)
                r.k[r.n_rb] = J.k;
                r.tiles[r.n_rb++] = J.ntiles;
            }
        }
        constexpr int NWp = 8;  // upper bound of waves per block across the pair-kernel geometries (stamp rows)
        const size_t nblk = (size_t)max_tiles * nj * B;
        if (ra.dbg & 32) ra.ts = stamp_buffer(h, nblk * NWp * 8, f.st);
        RbStreamPlan sp{};
        if (mode != 0 && rb_stream_supported(op, C, 1)) sp = rb_stream_plan(op, C, 1, sd, nj, (int)L, B, L * C, mode == 1, h->opt);
        if (sp.ok) {
            h->prof.launch(nms, flops, bytes, f.st, [&] { rb_stream_run(sp, f.st, h->opt); });
            r.pair_streamed |= 1 << m;
        } else {
            h->prof.launch(nm, flops, bytes, f.st, [&] { launch_rb_pair(op, C, ra, max_tiles, nj, B, max_rows, f.st); });
        }
        if ((ra.dbg & 32) && m == 0) print_stamps(h, nm, ra, nj, max_tiles, NWp, 8, nblk, f.st);  // (pair level 0)
        for (int j = 0; j < nk; ++j)
            if (dsts[j]) src[j] = dsts[j];
    }
    HIP_CHECK(hipGetLastError());
}

// ---- x = tanh(conv_post(leaky_relu(x)))                                    nsf.py:187-189
static void conv_post(const Fwd& f, const Act& x, float* out) {
    rvcmi_nsf* h = f.h;
    const int B = f.B, C = x.C, L = (int)x.L;
    hipStream_t st = f.st;
    const int dbg = h->opt.geti("POST_DBG", 0);
    h->prof.launch("conv_post", 2.0 * 7 * C * (double)x.L * B, (double)B * x.L * (C * h->cfg.n_resblock_kernels * (x.half ? 2 : 4) + 4), st, [&] {
        // round 6: three fp16 streams (every shipped config) through the LDS-DMA kernel: persistent blocks (3 per CU), next tile in flight
        // (option POST_DMA = 0: k_post)
        if (x.half && x.y[1] && x.y[2] && x.div == 3.f && (C == 32 || C == 16) && h->opt.geti("POST_DMA", 1) != 0) {
            const int ntiles = (L + POSTD_TT - 1) / POSTD_TT;
            const dim3 grid((unsigned)std::min(ntiles, std::max(1, num_cus() * 3 / B)), B);
            const _Float16* y0 = (const _Float16*)x.y[0];
            const _Float16* y1 = (const _Float16*)x.y[1];
            const _Float16* y2 = (const _Float16*)x.y[2];
            if (C == 32)
                hipLaunchKernelGGL(k_post_dma<32>, grid, dim3(POSTD_TT), post_dma_smem<32>(), st, y0, y1, y2, h->post_w.as<float>(), out, L, f.lens, x.lm, dbg);
            else
                hipLaunchKernelGGL(k_post_dma<16>, grid, dim3(POSTD_TT), post_dma_smem<16>(), st, y0, y1, y2, h->post_w.as<float>(), out, L, f.lens, x.lm, dbg);
            return;
        }
        const size_t smem = (size_t)(7 * C + (POST_TT + 6) * (C + 4)) * 4;
        hipLaunchKernelGGL(k_post, dim3((unsigned)((L + POST_TT - 1) / POST_TT), B), dim3(256), smem, st, x.y[0], x.y[1], x.y[2],
                           h->post_w.as<float>(), out, L, C, x.div, x.half ? 1 : 0, f.lens, x.lm, dbg);
    });
    HIP_CHECK(hipGetLastError());
}

// The fp32 [B][L][C] rows of X0 (the "up<i>" tap): an fp16 X0 is widened first.
static void tap_x0(const Fwd& f, const StagePlan& p, long L, int C) {
    rvcmi_nsf* h = f.h;
    if (!p.x0_half) return copy_tap_cl(h, h->X0.as<float>(), f.B, (int)L, C, f.tr, f.st);
    const size_t n = (size_t)f.B * L * C;
    hipLaunchKernelGGL(k_h2f, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, f.st, (const _Float16*)h->X0.p, h->Ya[0].as<float>(), n);
    copy_tap_cl(h, h->Ya[0].as<float>(), f.B, (int)L, C, f.tr, f.st);
}

// The un-divided sum of the stage's resblock outputs (the "stage<i>" tap).
static void tap_stage(const Fwd& f, const Act& x) {
    rvcmi_nsf* h = f.h;
    const size_t n = (size_t)f.B * x.L * x.C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (x.half)
        hipLaunchKernelGGL(k_sum3h, grid, dim3(256), 0, f.st, (const _Float16*)x.y[0], (const _Float16*)x.y[1], (const _Float16*)x.y[2],
                           h->X0.as<float>(), n);
    else
        hipLaunchKernelGGL(k_sum3, grid, dim3(256), 0, f.st, x.y[0], x.y[1], x.y[2], h->X0.as<float>(), n);
    copy_tap_cl(h, h->X0.as<float>(), f.B, (int)x.L, x.C, f.tr, f.st);
}

// `lens`: optional device array [B] of valid frames per item (1 <= lens[b] <= T): a ragged batch, every item computed exactly as
// a separate call of its own length (mfma_conv.hpp item_rows); the output rows behind an item's end are zero.
// `nres`: optional device array [B] of interpolation targets per item (1 <= nres[b] <= n_res, which is then their upper bound and the
// output's frame count): item b is interpolated to nres[b] frames and decoded as a ragged item of that length.
static void nsf_forward(rvcmi_nsf* h, int B, int T, const int* lens, const float* x, const float* f0, const float* g,
                        const float* noise, int n_res, float* out, hipStream_t st, TapRequest* tr, const int* nres = nullptr) {
    if (!h || !x || (!out && !tr)) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
    if (lens && n_res >= 0) RVCMI_FAIL(RVCMI_ERR_INVALID, "lengths and n_res (the realtime interpolation) cannot be combined");
    if (nres && (n_res < 1 || tr)) RVCMI_FAIL(RVCMI_ERR_INVALID, "per-item n_res needs n_res_max >= 1 and serves no debug tap");
    const rvcmi_nsf_config& c = h->cfg;
    if (c.use_f0 && !f0) RVCMI_FAIL(RVCMI_ERR_INVALID, "f0 is required for an NSF (use_f0) generator");
    if (B < 1 || T < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "B and T must be positive");
    const int Te = n_res >= 0 ? n_res : T;
    if (Te < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "n_res must be positive");
    if (B > h->max_B || T > h->max_T || Te > h->max_T)
        RVCMI_FAIL(RVCMI_ERR_NOMEM, "shape B=%d T=%d n_res=%d exceeds handle limits (max_B=%d max_T=%d)", B, T, n_res,
                   h->max_B, h->max_T);
    HIP_CHECK(hipSetDevice(h->device));
    Fwd f{h, c.operand, B, Te, lens, nres, nullptr, st, tr, nullptr};
    h->n_plan = 0;
    if (c.use_f0 && excitation(f, T, f0, noise)) return;
    if (nres) f.lens = nres;  // from conv_pre on, item b is a ragged item of nres[b] frames in rows of Te
    Act a = conv_pre(f, x, T, g);
    if (f.want("pre")) return copy_tap_cl(h, a.y[0], B, Te, h->C0, tr, st);
    char nm[48];
    for (int i = 0; i < c.n_ups; ++i) {
        const Stage& s = h->stages[i];
        const long L = a.L * s.u;
        const int lm = a.lm * s.u, C = s.cout;
        const StagePlan p = plan_stage(f, s, L, lm);
        f.rec = &h->last_plan[i];
        *f.rec = {(int)p.path, C, B, (int)L, p.x0_half, p.stage_half};  // (the resblock functions add what they launch with)
        f.rec->num_cus = num_cus();
        h->n_plan = i + 1;
        if (f.op == RVCMI_OPERAND_F32) ups_f32(f, s, a, L, lm);
        else ups_mfma(f, s, a, p, L, lm);
        snprintf(nm, sizeof(nm), "up%d", i);
        if (f.want(nm)) return tap_x0(f, p, L, C);
        const float* src[RVCMI_MAX_RB];
        for (auto& v : src) v = h->X0.as<float>();
        switch (p.path) {
            case RbPath::F32_CHAIN: rb_f32_chain(f, s, L, lm, src); break;
            case RbPath::SPLIT: rb_split(f, s, L, lm, src); break;
            case RbPath::STREAM: rb_stream(f, s, p, src); break;
            case RbPath::FULL: rb_full(f, s, p, L, lm, src); break;
            case RbPath::PAIR: rb_pair(f, s, L, lm, src); break;
        }
        const int nk = (int)s.rb.size();
        // x = xs / num_kernels (nsf.py:186) is applied by the consumer
        a = Act{{src[0], nk > 1 ? src[1] : nullptr, nk > 2 ? src[2] : nullptr}, p.stage_half, false, (float)nk, L, C, lm};
        snprintf(nm, sizeof(nm), "stage%d", i);
        if (f.want(nm)) return tap_stage(f, a);
    }
    if (tr) RVCMI_FAIL(RVCMI_ERR_INVALID, "unknown tap '%s'", tr->what);
    conv_post(f, a, out);
}

}  // namespace rvcmi

// ---- C ABI -------------------------------------------------------------------------------------
extern "C" {

int rvcmi_nsf_create(const rvcmi_nsf_config* cfg, const rvcmi_tensor* weights, int n_weights, int device, int max_B,
                     int max_T, rvcmi_nsf** out) {
    return guarded([&] { nsf_create(cfg, weights, n_weights, device, max_B, max_T, out); });
}
int rvcmi_nsf_destroy(rvcmi_nsf* h) {
    return guarded([&] { delete h; });
}
int rvcmi_nsf_forward(rvcmi_nsf* h, int B, int T, const int* lengths, const float* x, const float* f0, const float* g,
                      const float* noise, int n_res, float* out, void* stream) {
    return guarded([&] { nsf_forward(h, B, T, lengths, x, f0, g, noise, n_res, out, (hipStream_t)stream, nullptr); });
}
int rvcmi_nsf_forward_nres(rvcmi_nsf* h, int B, int T, int n_res_max, const int* n_res, const float* x, const float* f0, const float* g,
                           const float* noise, float* out, void* stream) {
    return guarded([&] {
        if (!n_res || n_res_max < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "forward_nres: n_res_dev is null or n_res_max = %d < 1", n_res_max);
        nsf_forward(h, B, T, nullptr, x, f0, g, noise, n_res_max, out, (hipStream_t)stream, nullptr, n_res);
    });
}
int rvcmi_nsf_upp(const rvcmi_nsf* h) { return h ? h->upp : RVCMI_ERR_INVALID; }
size_t rvcmi_nsf_workspace_bytes(const rvcmi_nsf* h) { return h ? h->ws_bytes : 0; }

int rvcmi_nsf_debug_forward(rvcmi_nsf* h, int B, int T, const float* x, const float* f0, const float* g,
                            const float* noise, int n_res, const char* what, float* out_host, size_t capacity_floats,
                            int64_t shape_out[3], void* stream) {
    return guarded([&] {
        if (!what || !out_host || !shape_out) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        TapRequest tr;
        tr.what = what;
        tr.out_host = out_host;
        tr.capacity = capacity_floats;
        tr.shape = shape_out;
        nsf_forward(h, B, T, nullptr, x, f0, g, noise, n_res, nullptr, (hipStream_t)stream, &tr);
        if (!tr.done) RVCMI_FAIL(RVCMI_ERR_INVALID, "tap '%s' was not produced", what);
    });
}

int rvcmi_nsf_set_option(rvcmi_nsf* h, const char* key, double value) {
    return guarded([&] {
        if (!h || !key) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        if ((!strcmp(key, "RBF_PAD_TAP") || !strcmp(key, "RBF32_TALL")) && value == value && value != 0.0 && value != 1.0)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "option '%s' takes 0 or 1", key);
        if (!strcmp(key, "RS_MFMA") && value == value && value != 16.0 && value != 32.0) RVCMI_FAIL(RVCMI_ERR_INVALID, "option 'RS_MFMA' takes 16 or 32");
        if (!h->opt.set(key, value)) RVCMI_FAIL(RVCMI_ERR_INVALID, "unknown option '%s' for this handle", key);
    });
}
int rvcmi_nsf_profile_enable(rvcmi_nsf* h, int enable) {
    return guarded([&] {
        if (!h) RVCMI_FAIL(RVCMI_ERR_INVALID, "null handle");
        h->prof.enabled = enable != 0;
    });
}
int rvcmi_nsf_last_plan(const rvcmi_nsf* h, rvcmi_nsf_stage_plan* out, int capacity, int* n) {
    return guarded([&] {
        if (!h || !n || (!out && h->n_plan)) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        if (capacity < h->n_plan) RVCMI_FAIL(RVCMI_ERR_INVALID, "capacity %d for the %d stages of the last forward", capacity, h->n_plan);
        std::copy(h->last_plan, h->last_plan + h->n_plan, out);
        *n = h->n_plan;
    });
}
int rvcmi_nsf_profile_read(rvcmi_nsf* h, rvcmi_kernel_stat* stats, int capacity, int* n, int reset) {
    return guarded([&] {
        if (!h) RVCMI_FAIL(RVCMI_ERR_INVALID, "null handle");
        h->prof.read(stats, capacity, n, reset);
    });
}

}  // extern "C"
