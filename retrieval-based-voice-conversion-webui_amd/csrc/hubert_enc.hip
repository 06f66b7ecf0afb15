// HuBERT's transformer encoder LAYERS (fairseq TransformerSentenceEncoderLayer with layer_norm_first = False = transformers
// HubertEncoderLayer) for gfx950: x = LN(x + Attn(x)); x = LN(x + FFN(x)), head dim 64, exact GELU.  Like csrc/hubert_fe.hip it is BEYOND
// the scope table of SURVEY.md section 8.  Kernels: hubert_enc_kernels.hpp.  A layer is FIVE launches, all enqueued on the caller's stream:
//     1  k_he_gemm<EPI_QKV>    [B T, d] x [d, 3 d] + bias, q scaled after the bias -> fp16 q / k / v, head-major
//     2  k_he_attn             online-softmax attention over key tiles, optional key mask -> fp16 [B T, d]
//     3  k_he_gemm_ln          out-projection + bias + residual + LayerNorm -> the stream (fp32, and fp16 as FFN-1's operand)
//     4  k_he_gemm<EPI_GELU>   FFN-1 + bias + exact GELU -> fp16 [B T, ffn]
//     5  k_he_gemm_ln          FFN-2 + bias + residual + LayerNorm -> the layer's output in the model's dtype
// The residual + LayerNorm sits in the GEMM's epilogue, not in a reduce kernel: a block owns 32 full rows, their accumulators spread over up to
// 16 waves.  Weights are packed once at create (q / k / v concatenated, everything fp16 in torch's [out][in] layout, which is K-contiguous).
// The forward allocates nothing.
#include <memory>
#include <string>

#include "common.hpp"
#include "hubert_enc_kernels.hpp"

using namespace rvcmi;
using namespace rvcmi::hubert_enc;

namespace {

constexpr int MAX_D = 1024, MAX_FFN = 4096, MAX_LAYERS = 64;
constexpr long long MAX_ROWS = 1ll << 22;  // B * T

struct Layer {
    DevBuf wqkv, bqkv, wo, bo, g1, b1, w1, bf1, w2, bf2, g2, b2;
};

struct Plan {
    size_t off_qkv, off_att, off_x1, off_x1h, off_h, off_tmp[2], bytes;
};

// B, T checked by the caller (B * T <= 2^22, d <= 1024, ffn <= 4096: every product below is under 2^36)
Plan plan_of(int B, int T, int d, int ffn) {
    Plan p;
    const size_t M = (size_t)B * T;
    Carve c;
    p.off_qkv = c.take(3 * M * d * 2);
    p.off_att = c.take(M * d * 2);
    p.off_x1 = c.take(M * d * 4);
    p.off_x1h = c.take(M * d * 2);
    p.off_h = c.take(M * ffn * 2);
    p.off_tmp[0] = c.take(M * d * 4);  // a layer's output on its way to the next (the model's dtype; fp32 is the larger)
    p.off_tmp[1] = c.take(M * d * 4);
    p.bytes = c.off;
    return p;
}

void check_shape(int B, int T, const char* who) {
    if (B < 1 || T < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: B = %d, T = %d (both at least 1)", who, B, T);
    if (B > 65535) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: B = %d items (at most 65535: one grid plane per item)", who, B);
    if ((long long)B * T > MAX_ROWS) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: B * T = %lld rows (at most 2^22)", who, (long long)B * T);
}

template <typename RT, typename OT, bool ALSO16>
void gemm_ln(const _Float16* x, const _Float16* w, const float* bias, const RT* res, const float* g, const float* b, float eps, OT* out, _Float16* out16,
             int M, int d, int K, hipStream_t st) {
    const dim3 grid((unsigned)((M + MT - 1) / MT));
    // as many waves as the columns allow (16 columns per wave at least): the weights stream through ceil(M / 32) blocks only
    if (d % 256 == 0)
        hipLaunchKernelGGL((k_he_gemm_ln<16, 4, RT, OT, ALSO16>), grid, dim3(1024), 0, st, x, w, bias, res, g, b, eps, out, out16, M, d, K);
    else if (d % 128 == 0)
        hipLaunchKernelGGL((k_he_gemm_ln<8, 8, RT, OT, ALSO16>), grid, dim3(512), 0, st, x, w, bias, res, g, b, eps, out, out16, M, d, K);
    else
        hipLaunchKernelGGL((k_he_gemm_ln<4, 16, RT, OT, ALSO16>), grid, dim3(256), 0, st, x, w, bias, res, g, b, eps, out, out16, M, d, K);
}

}  // namespace

struct rvcmi_hubert_enc {
    int device = 0, n_layers = 0, d = 0, heads = 0, ffn = 0;
    float eps = 1e-5f;
    std::vector<Layer> layers;
};

namespace {

// one layer: x (XT) -> out (XT)
template <typename XT>
void enqueue_layer(const rvcmi_hubert_enc* h, const Layer& L, const Plan& p, int B, int T, const XT* x, const uint8_t* mask, XT* out, char* ws, hipStream_t st) {
    const int M = B * T, d = h->d, H = h->heads, F = h->ffn;
    _Float16 *qkv = (_Float16*)(ws + p.off_qkv), *att = (_Float16*)(ws + p.off_att), *x1h = (_Float16*)(ws + p.off_x1h), *hb = (_Float16*)(ws + p.off_h);
    float* x1 = (float*)(ws + p.off_x1);
    const size_t one = (size_t)M * d;
    hipLaunchKernelGGL((k_he_gemm<XT, EPI_QKV>), dim3((unsigned)((M + GM - 1) / GM), (unsigned)((3 * d + GN - 1) / GN)), dim3(256), 0, st, x,
                       L.wqkv.as<_Float16>(), L.bqkv.as<float>(), qkv, M, 3 * d, d, T, H, 0.125f);
    hipLaunchKernelGGL(k_he_attn, dim3((unsigned)((T + QT - 1) / QT), (unsigned)H, (unsigned)B), dim3(256), 0, st, qkv, qkv + one, qkv + 2 * one, mask, att, T, H);
    gemm_ln<XT, float, true>(att, L.wo.as<_Float16>(), L.bo.as<float>(), x, L.g1.as<float>(), L.b1.as<float>(), h->eps, x1, x1h, M, d, d, st);
    hipLaunchKernelGGL((k_he_gemm<_Float16, EPI_GELU>), dim3((unsigned)((M + GM - 1) / GM), (unsigned)((F + GN - 1) / GN)), dim3(256), 0, st, x1h,
                       L.w1.as<_Float16>(), L.bf1.as<float>(), hb, M, F, d, T, H, 1.f);
    gemm_ln<float, XT, false>(hb, L.w2.as<_Float16>(), L.bf2.as<float>(), x1, L.g2.as<float>(), L.b2.as<float>(), h->eps, out, (_Float16*)nullptr, M, d, F, st);
}

template <typename XT>
void enqueue(const rvcmi_hubert_enc* h, const Plan& p, int first, int n, int B, int T, const void* x, const uint8_t* mask, void* out, char* ws, hipStream_t st) {
    const XT* cur = (const XT*)x;
    for (int i = 0; i < n; ++i) {
        XT* dst = i == n - 1 ? (XT*)out : (XT*)(ws + p.off_tmp[i & 1]);
        enqueue_layer<XT>(h, h->layers[first + i], p, B, T, cur, mask, dst, ws, st);
        cur = dst;
    }
}

}  // namespace

extern "C" {

int rvcmi_hubert_enc_create(const rvcmi_tensor* weights, int n_weights, int n_layers, int d, int heads, int ffn, float ln_eps, int device,
                            rvcmi_hubert_enc** out) {
    return guarded([&] {
        if (!weights || n_weights < 1 || !out) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_create: null argument");
        if (n_layers < 1 || n_layers > MAX_LAYERS) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_create: %d layers (1 .. %d)", n_layers, MAX_LAYERS);
        if (d < 64 || d > MAX_D || d % 64) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_create: d = %d (a multiple of 64 up to %d)", d, MAX_D);
        if (heads < 1 || heads * HD != d) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_create: %d heads of d = %d (the head dim must be 64)", heads, d);
        if (ffn < 64 || ffn > MAX_FFN || ffn % 64) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_create: FFN width %d (a multiple of 64 up to %d)", ffn, MAX_FFN);
        if (!(ln_eps > 0.f) || !(ln_eps < 1.f)) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_create: LayerNorm eps %g", (double)ln_eps);
        WeightTable wt(weights, n_weights, "hubert_enc_create");
        DeviceGuard dg(device);
        std::unique_ptr<rvcmi_hubert_enc> h(new rvcmi_hubert_enc());
        h->device = device, h->n_layers = n_layers, h->d = d, h->heads = heads, h->ffn = ffn, h->eps = ln_eps;
        h->layers.resize(n_layers);
        auto up32 = [](DevBuf& dst, const float* p, size_t n) { upload(dst, p, n * 4); };
        auto to16 = [](std::vector<_Float16>& v, size_t at, const float* p, size_t n) {
            for (size_t i = 0; i < n; ++i) v[at + i] = (_Float16)p[i];
        };
        const size_t dd = (size_t)d * d, df = (size_t)d * ffn;
        for (int l = 0; l < n_layers; ++l) {
            const std::string pre = "layers." + std::to_string(l) + ".";
            Layer& L = h->layers[l];
            std::vector<_Float16> wqkv(3 * dd), w(dd), wf(df);
            std::vector<float> bqkv(3 * (size_t)d);
            const char* names[3] = {"q_proj", "k_proj", "v_proj"};
            for (int i = 0; i < 3; ++i) {
                to16(wqkv, i * dd, wt.get(pre + "self_attn." + names[i] + ".weight", {d, d}), dd);
                memcpy(bqkv.data() + (size_t)i * d, wt.get(pre + "self_attn." + names[i] + ".bias", {d}), (size_t)d * 4);
            }
            upload(L.wqkv, wqkv);
            upload(L.bqkv, bqkv);
            to16(w, 0, wt.get(pre + "self_attn.out_proj.weight", {d, d}), dd);
            upload(L.wo, w);
            up32(L.bo, wt.get(pre + "self_attn.out_proj.bias", {d}), d);
            up32(L.g1, wt.get(pre + "self_attn_layer_norm.weight", {d}), d);
            up32(L.b1, wt.get(pre + "self_attn_layer_norm.bias", {d}), d);
            to16(wf, 0, wt.get(pre + "fc1.weight", {ffn, d}), df);
            upload(L.w1, wf);
            up32(L.bf1, wt.get(pre + "fc1.bias", {ffn}), ffn);
            to16(wf, 0, wt.get(pre + "fc2.weight", {d, ffn}), df);
            upload(L.w2, wf);
            up32(L.bf2, wt.get(pre + "fc2.bias", {d}), d);
            up32(L.g2, wt.get(pre + "final_layer_norm.weight", {d}), d);
            up32(L.b2, wt.get(pre + "final_layer_norm.bias", {d}), d);
        }
        wt.require_all_used("layer stack");  // a relative-position table, a seventeenth tensor of a layer ...
        *out = h.release();
    });
}

int rvcmi_hubert_enc_destroy(rvcmi_hubert_enc* h) {
    return guarded([&] { delete h; });
}

size_t rvcmi_hubert_enc_workspace_bytes(rvcmi_hubert_enc* h, int B, int T) {
    size_t n = 0;
    const int rc = guarded([&] {
        if (!h) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_workspace_bytes: null handle");
        check_shape(B, T, "hubert_enc_workspace_bytes");
        n = plan_of(B, T, h->d, h->ffn).bytes;
    });
    return rc == RVCMI_OK ? n : 0;
}

int rvcmi_hubert_enc_forward(rvcmi_hubert_enc* h, int first_layer, int n, int B, int T, const void* x_dev, int is_half, const uint8_t* key_mask_dev,
                             void* out_dev, void* ws_dev, void* stream) {
    return guarded([&] {
        if (!h || !x_dev || !out_dev || !ws_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_forward: null argument");
        if (((uintptr_t)ws_dev & 255) || ((uintptr_t)x_dev & 15) || ((uintptr_t)out_dev & 15))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_forward: the workspace must be 256-byte aligned, x and out 16-byte aligned");
        if (first_layer < 0 || n < 1 || first_layer > h->n_layers - n)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "hubert_enc_forward: layers %d .. %d + %d of %d", first_layer, first_layer, n, h->n_layers);
        check_shape(B, T, "hubert_enc_forward");
        const Plan p = plan_of(B, T, h->d, h->ffn);
        DeviceGuard dg(h->device);
        hipStream_t st = (hipStream_t)stream;
        if (is_half) enqueue<_Float16>(h, p, first_layer, n, B, T, x_dev, key_mask_dev, out_dev, (char*)ws_dev, st);
        else enqueue<float>(h, p, first_layer, n, B, T, x_dev, key_mask_dev, out_dev, (char*)ws_dev, st);
        HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
