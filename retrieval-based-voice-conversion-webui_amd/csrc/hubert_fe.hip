// HuBERT's convolutional feature extractor (fairseq ConvFeatureExtractionModel, extractor_mode "default" = transformers
// HubertFeatureEncoder with feat_extract_norm "group") for gfx950: the seven bias-free Conv1d layers in front of the transformer,
//     layer 0      1 -> 512, k 10, stride 5, GroupNorm(512 groups, eps 1e-5, affine), exact GELU
//     layers 1 - 4 512 -> 512, k 3, stride 2, exact GELU
//     layers 5 - 6 512 -> 512, k 2, stride 2, exact GELU
// [B][N] samples -> [B][L6][512] fp16, L6 = (N - 400) / 320 + 1.  Like csrc/unet.hip it is BEYOND the scope table of SURVEY.md section 8.
// Kernels: hubert_fe_kernels.hpp.  Weights are packed once at create ([Cout][tap][Cin] fp16: K = tap x channel is contiguous in both GEMM
// operands).  A forward is five launches for layer 0's statistics and pass plus one per later layer, all enqueued on the caller's stream.
// rvcmi_hubert_fe_forward_ragged runs the same launches on a [B][N_max] batch whose items have lengths of their own (the kernels' RAGGED
// instantiations): buffers and grids are those of N_max, every item's rows are those of its lone call.
#include <memory>
#include <string>

#include "common.hpp"
#include "hubert_fe_kernels.hpp"

using namespace rvcmi;
using namespace rvcmi::hubert;

struct rvcmi_hubert_fe;

namespace {

constexpr int NLAYERS = 7;
constexpr int TAPS[NLAYERS] = {10, 3, 3, 3, 3, 2, 2};
constexpr double GN_EPS = 1e-5;
constexpr int MAX_N = 1 << 30;

int frames_of(long long N) { return N < 400 ? 0 : (int)((N - 400) / 320 + 1); }

// rows after layer l (0 .. 6) of an N-sample input
void layer_rows(int N, int* L) {
    L[0] = (N - K0) / S0 + 1;
    for (int l = 1; l < NLAYERS; ++l) L[l] = (L[l - 1] - TAPS[l]) / 2 + 1;
}

struct Plan {
    int L[NLAYERS];
    int nchunk;
    size_t off_a, off_b, off_part, off_meanf, off_scale, off_shift, bytes;
};

// B >= 1, 400 <= N <= 2^30 checked by the caller
Plan plan_of(int B, int N) {
    Plan p;
    layer_rows(N, p.L);
    p.nchunk = (p.L[0] + ST_FRAMES - 1) / ST_FRAMES;
    Carve c;
    p.off_a = c.take((size_t)B * p.L[0] * HC * 2);  // outputs of layers 0, 2, 4
    p.off_b = c.take((size_t)B * p.L[1] * HC * 2);  // outputs of layers 1, 3, 5
    p.off_part = c.take((size_t)B * p.nchunk * ST_VALS * sizeof(double));
    p.off_meanf = c.take((size_t)B * K0 * 4);
    p.off_scale = c.take((size_t)B * HC * 4);
    p.off_shift = c.take((size_t)B * HC * 4);
    p.bytes = c.off;
    return p;
}

void check_shape(int B, long long N, const char* who) {
    if (B < 1 || N < 400) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: B = %d, N = %lld (B >= 1, N >= 400: one output frame)", who, B, N);
    if (B > 65535) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: B = %d items (at most 65535: one grid row per item)", who, B);
    if (N > MAX_N) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: N = %lld samples (at most 2^30)", who, N);
}

// torch Conv1d weight [512][512][taps] -> [512][taps][512] fp16
std::vector<_Float16> pack_conv(const float* w, int taps) {
    std::vector<_Float16> o((size_t)HC * taps * HC);
    for (int co = 0; co < HC; ++co)
        for (int ci = 0; ci < HC; ++ci)
            for (int t = 0; t < taps; ++t) o[((size_t)co * taps + t) * HC + ci] = (_Float16)w[((size_t)co * HC + ci) * taps + t];
    return o;
}

// lens == NULL: dense.  Else layer ``layer`` of the ragged batch (Lin: the longest item's rows, the stride); ``zero_tail``: the last layer.
void gemm(const _Float16* x, const _Float16* w, void* out, int B, int Lin, int taps, bool out32, hipStream_t st, const int* lens = nullptr, int layer = 0,
          bool zero_tail = false) {
    const int Lout = (Lin - taps) / 2 + 1;
    const dim3 grid((unsigned)((Lout + GM - 1) / GM), HC / GN, (unsigned)B);
    if (lens) hipLaunchKernelGGL((k_hfe_gemm<false, true>), grid, dim3(256), 0, st, x, w, out, Lin, Lout, taps * HC, lens, layer, zero_tail ? 1 : 0);
    else if (out32) hipLaunchKernelGGL((k_hfe_gemm<true, false>), grid, dim3(256), 0, st, x, w, out, Lin, Lout, taps * HC, (const int*)nullptr, 0, 0);
    else hipLaunchKernelGGL((k_hfe_gemm<false, false>), grid, dim3(256), 0, st, x, w, out, Lin, Lout, taps * HC, (const int*)nullptr, 0, 0);
}

// the launches of one forward; lens == NULL: dense (N is every item's length), else ragged (N = N_max, the strides)
template <bool RAGGED>
void enqueue(rvcmi_hubert_fe* h, const Plan& p, int B, size_t N, const int* lens, const void* x_dev, int x_is_half, void* out16_dev, char* ws, hipStream_t st);

}  // namespace

struct rvcmi_hubert_fe {
    int device = 0;
    DevBuf w0, gamma, beta, w[NLAYERS];  // w0: [512][10] fp32 holding the fp16-rounded values; w[1 .. 6]: packed fp16
    GrowBuf ws;                          // the handle's own workspace (forward with ws_dev == NULL)
};

namespace {

template <bool RAGGED>
void enqueue(rvcmi_hubert_fe* h, const Plan& p, int B, size_t N, const int* lens, const void* x_dev, int x_is_half, void* out16_dev, char* ws, hipStream_t st) {
    _Float16 *A = (_Float16*)(ws + p.off_a), *Bb = (_Float16*)(ws + p.off_b);
    double* part = (double*)(ws + p.off_part);
    float *meanf = (float*)(ws + p.off_meanf), *scale = (float*)(ws + p.off_scale), *shift = (float*)(ws + p.off_shift);
    const int L0 = p.L[0];
    const dim3 gs((unsigned)p.nchunk, (unsigned)B), g0((unsigned)((L0 + F0_BLK - 1) / F0_BLK), (unsigned)B);
    if (x_is_half) hipLaunchKernelGGL((k_hfe_stats<_Float16, RAGGED>), gs, dim3(256), 0, st, (const _Float16*)x_dev, N, L0, part, lens);
    else hipLaunchKernelGGL((k_hfe_stats<float, RAGGED>), gs, dim3(256), 0, st, (const float*)x_dev, N, L0, part, lens);
    hipLaunchKernelGGL(k_hfe_stats_final<RAGGED>, dim3((unsigned)B), dim3(HC), 0, st, part, p.nchunk, L0, h->w0.as<float>(), h->gamma.as<float>(),
                       h->beta.as<float>(), GN_EPS, meanf, scale, shift, lens);
    if (x_is_half)
        hipLaunchKernelGGL((k_hfe_conv0<_Float16, RAGGED>), g0, dim3(256), 0, st, (const _Float16*)x_dev, N, L0, h->w0.as<float>(), meanf, scale, shift, A,
                           lens);
    else
        hipLaunchKernelGGL((k_hfe_conv0<float, RAGGED>), g0, dim3(256), 0, st, (const float*)x_dev, N, L0, h->w0.as<float>(), meanf, scale, shift, A, lens);
    _Float16* cur = A;
    for (int l = 1; l < NLAYERS; ++l) {
        _Float16* dst = l == NLAYERS - 1 ? (_Float16*)out16_dev : (cur == A ? Bb : A);
        gemm(cur, h->w[l].as<_Float16>(), dst, B, p.L[l - 1], TAPS[l], false, st, RAGGED ? lens : nullptr, l, l == NLAYERS - 1);
        cur = dst;
    }
}

}  // namespace

extern "C" {

int rvcmi_hubert_fe_create(const rvcmi_tensor* weights, int n_weights, int device, rvcmi_hubert_fe** out) {
    return guarded([&] {
        if (!weights || n_weights < 1 || !out) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_fe_create: null argument");
        WeightTable wt(weights, n_weights, "hubert_fe_create");
        const float* wl[NLAYERS];
        for (int l = 0; l < NLAYERS; ++l) wl[l] = wt.get("conv_layers." + std::to_string(l) + ".0.weight", {HC, l ? HC : 1, TAPS[l]});
        const float *g = wt.get("conv_layers.0.2.weight", {HC}), *bt = wt.get("conv_layers.0.2.bias", {HC});
        wt.require_all_used("extractor");  // a conv bias, an eighth layer, a norm behind another layer ...
        DeviceGuard dg(device);
        std::unique_ptr<rvcmi_hubert_fe> h(new rvcmi_hubert_fe());
        h->device = device;
        std::vector<float> w0((size_t)HC * K0);
        for (size_t i = 0; i < w0.size(); ++i) w0[i] = (float)(_Float16)wl[0][i];
        upload(h->w0, w0);
        upload(h->gamma, g, HC * 4);
        upload(h->beta, bt, HC * 4);
        for (int l = 1; l < NLAYERS; ++l) upload(h->w[l], pack_conv(wl[l], TAPS[l]));
        *out = h.release();
    });
}

int rvcmi_hubert_fe_destroy(rvcmi_hubert_fe* h) {
    return guarded([&] { delete h; });
}

int64_t rvcmi_hubert_fe_frames(int64_t N) { return N > MAX_N ? 0 : frames_of(N); }

size_t rvcmi_hubert_fe_workspace_bytes(rvcmi_hubert_fe* h, int B, int64_t N) {
    size_t n = 0;
    const int rc = guarded([&] {
        if (!h) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_fe_workspace_bytes: null handle");
        check_shape(B, N, "hubert_fe_workspace_bytes");
        n = plan_of(B, (int)N).bytes;
    });
    return rc == RVCMI_OK ? n : 0;
}

int rvcmi_hubert_fe_forward(rvcmi_hubert_fe* h, int B, int64_t N, const void* x_dev, int x_is_half, void* out16_dev, void* ws_dev, void* stream) {
    return guarded([&] {
        if (!h || !x_dev || !out16_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_fe_forward: null argument");
        check_shape(B, N, "hubert_fe_forward");
        const Plan p = plan_of(B, (int)N);
        DeviceGuard dg(h->device);
        hipStream_t st = (hipStream_t)stream;
        char* ws = ws_dev ? (char*)ws_dev : h->ws.ensure(p.bytes, st);
        enqueue<false>(h, p, B, (size_t)N, nullptr, x_dev, x_is_half, out16_dev, ws, st);
        HIP_CHECK(hipGetLastError());
    });
}

size_t rvcmi_hubert_fe_workspace_bytes_ragged(rvcmi_hubert_fe* h, int B, int64_t N_max) {
    size_t n = 0;
    const int rc = guarded([&] {
        if (!h) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_fe_workspace_bytes_ragged: null handle");
        check_shape(B, N_max, "hubert_fe_workspace_bytes_ragged");
        n = plan_of(B, (int)N_max).bytes;
    });
    return rc == RVCMI_OK ? n : 0;
}

int rvcmi_hubert_fe_forward_ragged(rvcmi_hubert_fe* h, int B, int64_t N_max, const int* lens_host, const int* lens_dev, const void* x_dev, int x_is_half,
                                   void* out16_dev, void* ws_dev, void* stream) {
    return guarded([&] {
        if (!h || !x_dev || !out16_dev || !lens_host || !lens_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_fe_forward_ragged: null argument");
        check_shape(B, N_max, "hubert_fe_forward_ragged");
        bool full = false;
        for (int i = 0; i < B; ++i) {
            if (lens_host[i] < 400 || lens_host[i] > N_max)
                RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_fe_forward_ragged: item %d has %d samples (400 .. N_max = %lld)", i, lens_host[i], (long long)N_max);
            full = full || lens_host[i] == N_max;
        }
        if (!full) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_fe_forward_ragged: no item is N_max = %lld samples long", (long long)N_max);
        const Plan p = plan_of(B, (int)N_max);
        DeviceGuard dg(h->device);
        hipStream_t st = (hipStream_t)stream;
        char* ws = ws_dev ? (char*)ws_dev : h->ws.ensure(p.bytes, st);
        enqueue<true>(h, p, B, (size_t)N_max, lens_dev, x_dev, x_is_half, out16_dev, ws, st);
        HIP_CHECK(hipGetLastError());
    });
}

int rvcmi_hubert_fe_debug_conv(int taps, int B, int L_in, const float* w, const void* x16_dev, float* out32_dev, int device, void* stream) {
    return guarded([&] {
        if ((taps != 2 && taps != 3) || B < 1 || B > 65535 || L_in < taps || (long long)B * L_in > (1ll << 24) || !w || !x16_dev || !out32_dev)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_fe_debug_conv: bad argument");
        DeviceGuard dg(device);
        hipStream_t st = (hipStream_t)stream;
        const std::vector<_Float16> p = pack_conv(w, taps);
        DevBuf wd;
        upload(wd, p);
        gemm((const _Float16*)x16_dev, wd.as<_Float16>(), out32_dev, B, L_in, taps, true, st);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

}  // extern "C"
