// The deep U-Net of the RMVPE f0 network and its 3-channel head (rvc/f0/deepunet.py, rvc/f0/e2e.py:21-29,44-46) for gfx950: everything
// E2E.forward does between the transposed mel input and the GRU's input.  Like csrc/gru.hip it is BEYOND the scope table of SURVEY.md
// section 8; bench.py --e2e measured this part at 6.5 ms of a 17-20 ms conversion on PyTorch-ROCm / MIOpen (117 convolutions with unfused
// BatchNorm, ReLU, residual add, pooling and concatenation).
//
// Geometry comes from the weights (state-dict names under "unet." and "cnn."): encoder / decoder levels, units per level, intermediate
// layers, base channel count.  Supported: one input channel, 128 mel bins, pooling (2, 2), every channel count a multiple of 16.
//
// A ConvBlockRes unit is three launches (kernels: unet_kernels.hpp):
//     t = relu(bn1(conv3x3(x)))                       k_unet_conv
//     s = shortcut1x1(x) + bias   (first unit only)   k_unet_conv, 1 tap
//     y = relu(bn2(conv3x3(t))) + (s or x)            k_unet_conv, residual added after the ReLU
// The first unit of a decoder level reads (upsampled, skip) as two sources.  Layers with few pixels (the 256 / 512-channel levels of a short
// window stream megabytes of weights for a handful of pixels) split their K loop over blocks and reduce the fp32 partials in fixed order.
// The handle owns the packed weights only; activations, skip tensors and partials live in the caller's workspace
// (rvcmi_unet_workspace_bytes), so a forward neither allocates nor frees: it is safe inside a stream capture.
#include <memory>
#include <string>

#include "common.hpp"
#include "unet_kernels.hpp"

using namespace rvcmi;
using namespace rvcmi::unet;

namespace {

constexpr int NMEL = 128;
constexpr double BN_EPS = 1e-5;  // torch.nn.BatchNorm2d default, which deepunet.py keeps

struct Conv {
    size_t w = 0, scale = 0, shift = 0;  // byte offsets into the weight arena
    int Cin = 0, Cout = 0, mode = MODE_3X3;
};
struct Unit {
    Conv c1, c2, sc;
    bool has_sc = false;
};

struct Arena {
    std::vector<char> host;
    size_t push(const void* p, size_t bytes) {
        const size_t o = align256(host.size());
        host.resize(o + bytes);
        memcpy(host.data() + o, p, bytes);
        return o;
    }
    size_t push_f32(const std::vector<float>& v) { return push(v.data(), v.size() * 4); }
    size_t push_f16(const std::vector<_Float16>& v) { return push(v.data(), v.size() * 2); }
};

std::vector<float> padded16(const float* p, int n, float fill) {
    std::vector<float> v((size_t)((n + 15) / 16 * 16), fill);
    for (int i = 0; i < n; ++i) v[i] = p[i];
    return v;
}

// torch Conv2d weight [Cout][Cin][k][k] -> [Cout][tap][Cin] fp16
std::vector<_Float16> pack_conv(const float* w, int Cout, int Cin, int k) {
    std::vector<_Float16> o((size_t)Cout * k * k * Cin);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < k * k; ++t) o[((size_t)co * k * k + t) * Cin + ci] = (_Float16)w[((size_t)co * Cin + ci) * k * k + t];
    return o;
}

// torch ConvTranspose2d weight [Cin][Cout][3][3] -> the four output phases (py, px), each [Cout][tap][Cin]: tap (ty, tx) of a phase with
// two taps along an axis is kernel index 0 (input + 1) then 2 (input + 0); a phase with one tap takes kernel index 1
std::vector<_Float16> pack_up(const float* w, int Cin, int Cout) {
    std::vector<_Float16> o((size_t)9 * Cout * Cin);
    size_t base = 0;
    for (int ph = 0; ph < 4; ++ph) {
        const int py = ph >> 1, px = ph & 1, nty = up_taps(py), ntx = up_taps(px);
        for (int co = 0; co < Cout; ++co)
            for (int ty = 0; ty < nty; ++ty)
                for (int tx = 0; tx < ntx; ++tx) {
                    const int ky = py ? (ty == 0 ? 0 : 2) : 1, kx = px ? (tx == 0 ? 0 : 2) : 1;
                    for (int ci = 0; ci < Cin; ++ci)
                        o[base + ((size_t)co * nty * ntx + ty * ntx + tx) * Cin + ci] = (_Float16)w[(((size_t)ci * Cout + co) * 3 + ky) * 3 + kx];
                }
        base += (size_t)nty * ntx * Cout * Cin;
    }
    return o;
}

struct Ctx {
    const char* wbase = nullptr;  // device weight arena
    hipStream_t st = nullptr;
    bool dry = false;             // size the workspace / check the grids only
    int force_ksplit = 0;
    float* part = nullptr;
    size_t max_part = 0;
    const int* seq_off = nullptr;  // ragged: device offsets of the packed sequences (unet_kernels.hpp), R = rows at level 0
    int nseq = 0, R = 0;
};

// level of an image of H rows in a ragged forward of c.R rows
int level_of(const Ctx& c, int H) {
    int l = 0;
    while ((c.R >> l) > H) ++l;
    return l;
}

void check_grid(unsigned long long gx, unsigned long long gy, unsigned long long gz) {
    if (gx == 0 || gy == 0 || gz == 0 || gx > 2147483647ull || gy > 65535ull || gz > 65535ull)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "unet: a launch of %llu x %llu x %llu blocks exceeds the grid limits", gx, gy, gz);
}

void conv(Ctx& c, const Conv& L, const _Float16* x0, int C0, const _Float16* x1, int C1, int B, int H, int W, int relu, const _Float16* res, void* out,
          int out_kind) {
    if (C0 + C1 != L.Cin || C0 % 8 || C1 % 8) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet: channel mismatch (%d + %d into a layer of %d)", C0, C1, L.Cin);
    const long long M = (long long)B * H * W;
    const int cfg = L.Cout <= 16 ? 0 : L.Cout <= 32 ? 1 : 2;
    const int pix_blk = cfg == 2 ? 64 : 128, co_blk = cfg == 0 ? 16 : cfg == 1 ? 32 : 64;
    const unsigned long long gx = (unsigned long long)((M + pix_blk - 1) / pix_blk), gy = (unsigned long long)((L.Cout + co_blk - 1) / co_blk);
    const int phases = L.mode == MODE_UP ? 4 : 1;
    const int nch = (L.Cin + 31) / 32, ntaps = L.mode == MODE_3X3 ? 9 : L.mode == MODE_UP ? 4 : 1;
    int ksplit = 1;
    if (out_kind == OUT_NHWC16 && L.Cout % 16 == 0) {
        const unsigned long long blocks = gx * gy * phases;
        if (c.force_ksplit > 0) ksplit = c.force_ksplit;
        else if (blocks < 128) ksplit = (int)std::min<unsigned long long>(std::min<unsigned long long>((256 + blocks - 1) / blocks, 32), std::max(1, ntaps * nch / 4));
    }
    check_grid(gx, gy, (unsigned long long)phases * ksplit);
    const long long Mo = L.mode == MODE_UP ? 4 * M : M;
    if (ksplit > 1) c.max_part = std::max(c.max_part, (size_t)((size_t)ksplit * (size_t)Mo * L.Cout * 4));
    if (c.dry) return;
    ConvArgs a;
    a.x0 = x0;
    a.x1 = x1;
    a.w = (const _Float16*)(c.wbase + L.w);
    a.scale = (const float*)(c.wbase + L.scale);
    a.shift = (const float*)(c.wbase + L.shift);
    a.res = res;
    a.out = out;
    a.part = c.part;
    a.B = B, a.H = H, a.W = W, a.C0 = C0, a.C1 = C1, a.Cout = L.Cout, a.mode = L.mode, a.relu = relu, a.ksplit = ksplit, a.out_kind = out_kind;
    a.seq_off = c.seq_off, a.nseq = c.nseq, a.seq_shift = c.seq_off ? level_of(c, H) : 0;
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)(phases * ksplit));
    if (cfg == 0) hipLaunchKernelGGL((k_unet_conv<1, 1>), grid, dim3(256), 0, c.st, a);
    else if (cfg == 1) hipLaunchKernelGGL((k_unet_conv<2, 1>), grid, dim3(256), 0, c.st, a);
    else hipLaunchKernelGGL((k_unet_conv<2, 2>), grid, dim3(256), 0, c.st, a);
    if (ksplit > 1) {
        const size_t n4 = (size_t)Mo * L.Cout / 4;
        hipLaunchKernelGGL(k_unet_reduce, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, c.st, c.part, ksplit, n4, L.Cout, a.scale, a.shift, relu, res,
                           (_Float16*)out);
    }
}

void first(Ctx& c, const Conv& L, int ntaps, const float* x, float in_scale, float in_shift, int relu, _Float16* out, int B, int H, int W) {
    const unsigned long long n = (unsigned long long)B * H * W * (L.Cout / 8), gx = (n + 255) / 256;
    check_grid(gx, 1, 1);
    if (c.dry) return;
    hipLaunchKernelGGL(k_unet_first, dim3((unsigned)gx), dim3(256), 0, c.st, x, in_scale, in_shift, (const _Float16*)(c.wbase + L.w), ntaps,
                       (const float*)(c.wbase + L.scale), (const float*)(c.wbase + L.shift), relu, out, B, H, W, L.Cout, c.seq_off, c.nseq);
}

void pool(Ctx& c, const _Float16* x, _Float16* out, int B, int H, int W, int C) {
    const unsigned long long n = (unsigned long long)B * (H / 2) * (W / 2) * (C / 8), gx = (n + 255) / 256;
    check_grid(gx, 1, 1);
    if (c.dry) return;
    hipLaunchKernelGGL(k_unet_pool, dim3((unsigned)gx), dim3(256), 0, c.st, x, out, B, H, W, C);
}

}  // namespace

struct rvcmi_unet {
    int device = 0, levels = 0, blocks = 0, inters = 0, base = 0;
    float in_scale = 1.f, in_shift = 0.f;
    DevBuf arena;
    std::vector<std::vector<Unit>> enc, inter, dec;
    std::vector<Conv> up;
    Conv head;
};

namespace {

struct Loader {
    WeightTable wt;
    Arena arena;

    bool has(const std::string& n) const { return wt.has(n); }
    const float* get(const std::string& n, std::initializer_list<int64_t> shape) { return wt.get(n, shape); }
    // eval-mode BatchNorm as y = x * scale + shift
    void bn(const std::string& p, int C, std::vector<float>& scale, std::vector<float>& shift) {
        const float *g = get(p + ".weight", {C}), *b = get(p + ".bias", {C}), *m = get(p + ".running_mean", {C}), *v = get(p + ".running_var", {C});
        scale.assign((size_t)((C + 15) / 16 * 16), 1.f);
        shift.assign(scale.size(), 0.f);
        for (int i = 0; i < C; ++i) {
            const double s = (double)g[i] / sqrt((double)v[i] + BN_EPS);
            scale[i] = (float)s;
            shift[i] = (float)((double)b[i] - (double)m[i] * s);
        }
    }
    Conv conv_bn(const std::string& wname, const std::string& bnname, int Cin, int Cout) {
        Conv c;
        c.Cin = Cin, c.Cout = Cout, c.mode = MODE_3X3;
        c.w = arena.push_f16(pack_conv(get(wname, {Cout, Cin, 3, 3}), Cout, Cin, 3));
        std::vector<float> sc, sh;
        bn(bnname, Cout, sc, sh);
        c.scale = arena.push_f32(sc);
        c.shift = arena.push_f32(sh);
        return c;
    }
    Unit unit(const std::string& p, int Cin, int Cout) {
        if (Cout % 16 || (Cin != 1 && Cin % 16)) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_create: '%s' has %d -> %d channels (multiples of 16 only)", p.c_str(), Cin, Cout);
        Unit u;
        u.c1 = conv_bn(p + ".conv.0.weight", p + ".conv.1", Cin, Cout);
        u.c2 = conv_bn(p + ".conv.3.weight", p + ".conv.4", Cout, Cout);
        u.has_sc = Cin != Cout;
        if (u.has_sc) {
            u.sc.Cin = Cin, u.sc.Cout = Cout, u.sc.mode = MODE_1X1;
            u.sc.w = arena.push_f16(pack_conv(get(p + ".shortcut.weight", {Cout, Cin, 1, 1}), Cout, Cin, 1));
            u.sc.scale = arena.push_f32(std::vector<float>((size_t)((Cout + 15) / 16 * 16), 1.f));
            u.sc.shift = arena.push_f32(padded16(get(p + ".shortcut.bias", {Cout}), Cout, 0.f));
        }
        return u;
    }
};

std::string idx(const char* fmt, int a, int b = 0) {
    char buf[160];
    snprintf(buf, sizeof buf, fmt, a, b);
    return buf;
}

bool shape_ok(const rvcmi_unet* h, int B, int T) {
    return h && B >= 1 && T >= (1 << h->levels) && T % (1 << h->levels) == 0 && (long long)B * T <= (1ll << 22);
}

// A ragged batch: nseq >= 1 sequences, off[0] == 0, every length off[i + 1] - off[i] a positive multiple of 2^levels, R = off[nseq] <= 2^22
void check_ragged(const rvcmi_unet* h, int nseq, const int* off, const char* who) {
    if (!h || !off || nseq < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: %d sequences", who, nseq);
    const int step = 1 << h->levels;
    if (off[0] != 0) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: the first offset is %d, not 0", who, off[0]);
    for (int i = 0; i < nseq; ++i) {
        const long long len = (long long)off[i + 1] - off[i];
        if (len < step || len % step)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: sequence %d has %lld rows (offsets must ascend by multiples of %d)", who, i, len, step);
        if (off[i + 1] > (1 << 22)) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: more than 2^22 rows", who);
    }
}

// Enqueues (or, dry, sizes and checks) one forward.  -> workspace bytes.  seq_off_dev / nseq: a ragged forward (B = 1, T = all packed rows).
size_t run(const rvcmi_unet* h, int B, int T, const float* mel, float* out, char* ws, hipStream_t st, bool dry, const int* seq_off_dev = nullptr,
           int nseq = 0) {
    Ctx c;
    c.wbase = h->arena.as<char>();
    c.st = st;
    c.dry = dry;
    c.seq_off = seq_off_dev, c.nseq = nseq, c.R = T;
    Carve carve;
    auto take = [&](size_t bytes) { return (_Float16*)(ws + carve.take(bytes)); };
    const int L = h->levels;
    const size_t full = (size_t)B * T * NMEL * h->base * 2;
    _Float16 *X0 = take(full), *X1 = take(full), *Tb = take(full), *Sb = take(full);
    std::vector<_Float16*> skip(L);
    for (int l = 0; l < L; ++l) skip[l] = take(((size_t)B * (T >> l) * (NMEL >> l) * ((size_t)h->base << l)) * 2);
    c.part = (float*)(ws + carve.off);
    auto other = [&](const _Float16* p) { return p == X0 ? X1 : X0; };
    auto unit = [&](const Unit& u, const _Float16* x0, int C0, const _Float16* x1, int C1, int H, int W, _Float16* dst) {
        conv(c, u.c1, x0, C0, x1, C1, B, H, W, 1, nullptr, Tb, OUT_NHWC16);
        const _Float16* res = x0;
        if (u.has_sc) {
            conv(c, u.sc, x0, C0, x1, C1, B, H, W, 0, nullptr, Sb, OUT_NHWC16);
            res = Sb;
        }
        conv(c, u.c2, Tb, u.c2.Cin, nullptr, 0, B, H, W, 1, res, dst, OUT_NHWC16);
    };
    int H = T, W = NMEL, C = 1;
    _Float16* cur = nullptr;
    for (int l = 0; l < L; ++l) {
        const int nu = (int)h->enc[l].size();
        for (int u = 0; u < nu; ++u) {
            const Unit& U = h->enc[l][u];
            _Float16* dst = u == nu - 1 ? skip[l] : other(cur);
            if (l == 0 && u == 0) {  // one input channel, behind the input BatchNorm
                first(c, U.c1, 9, mel, h->in_scale, h->in_shift, 1, Tb, B, H, W);
                first(c, U.sc, 1, mel, h->in_scale, h->in_shift, 0, Sb, B, H, W);
                conv(c, U.c2, Tb, U.c2.Cin, nullptr, 0, B, H, W, 1, Sb, dst, OUT_NHWC16);
            } else {
                unit(U, cur, C, nullptr, 0, H, W, dst);
            }
            cur = dst;
            C = U.c2.Cout;
        }
        pool(c, cur, X0, B, H, W, C);
        cur = X0;
        H >>= 1, W >>= 1;
    }
    for (const auto& layer : h->inter)
        for (const Unit& U : layer) {
            _Float16* dst = other(cur);
            unit(U, cur, C, nullptr, 0, H, W, dst);
            cur = dst;
            C = U.c2.Cout;
        }
    for (int i = 0; i < L; ++i) {
        _Float16* U0 = other(cur);
        conv(c, h->up[i], cur, C, nullptr, 0, B, H, W, 1, nullptr, U0, OUT_NHWC16);
        H <<= 1, W <<= 1, C = h->up[i].Cout;
        const _Float16* x = U0;
        for (size_t u = 0; u < h->dec[i].size(); ++u) {
            const Unit& U = h->dec[i][u];
            _Float16* dst = u == 0 ? cur : other(x);
            if (u == 0) unit(U, x, C, skip[L - 1 - i], C, H, W, dst);
            else unit(U, x, C, nullptr, 0, H, W, dst);
            x = dst;
        }
        cur = const_cast<_Float16*>(x);
    }
    conv(c, h->head, cur, C, nullptr, 0, B, H, W, 0, nullptr, out, OUT_HEAD32);
    if (!dry) HIP_CHECK(hipGetLastError());
    return carve.off + align256(c.max_part);
}

}  // namespace

extern "C" {

int rvcmi_unet_create(const rvcmi_tensor* weights, int n_weights, int device, rvcmi_unet** out) {
    return guarded([&] {
        if (!weights || n_weights < 1 || !out) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_create: null argument");
        Loader ld{WeightTable(weights, n_weights, "unet_create"), {}};
        std::unique_ptr<rvcmi_unet> h(new rvcmi_unet());
        h->device = device;
        const std::string w00 = "unet.encoder.layers.0.conv.0.conv.0.weight";
        const rvcmi_tensor* t0 = ld.wt.find(w00);
        if (!t0) RVCMI_FAIL(RVCMI_ERR_MISSING, "unet_create: missing weight tensor '%s'", w00.c_str());
        if (t0->ndim != 4 || t0->shape[1] != 1 || t0->shape[0] < 16 || t0->shape[0] > 4096 || t0->shape[0] % 16)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_create: the first layer must map 1 channel to a multiple of 16");
        h->base = (int)t0->shape[0];
        while (ld.has(idx("unet.encoder.layers.%d.conv.0.conv.0.weight", h->levels))) ++h->levels;
        while (ld.has(idx("unet.encoder.layers.0.conv.%d.conv.0.weight", h->blocks))) ++h->blocks;
        while (ld.has(idx("unet.intermediate.layers.%d.conv.0.conv.0.weight", h->inters))) ++h->inters;
        if (h->levels < 1 || h->levels > 7 || h->inters < 1 || (long long)h->base << h->levels > 65536)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_create: %d levels / %d intermediate layers / %d base channels not supported", h->levels, h->inters, h->base);
        {   // Encoder.bn: BatchNorm2d(1) in front of the first convolution's zero padding
            std::vector<float> sc, sh;
            ld.bn("unet.encoder.bn", 1, sc, sh);
            h->in_scale = sc[0], h->in_shift = sh[0];
        }
        int cin = 1, cout = h->base;
        for (int l = 0; l < h->levels; ++l) {
            h->enc.emplace_back();
            for (int u = 0; u < h->blocks; ++u) h->enc[l].push_back(ld.unit(idx("unet.encoder.layers.%d.conv.%d", l, u), u ? cout : cin, cout));
            cin = cout, cout *= 2;
        }
        for (int i = 0; i < h->inters; ++i) {
            h->inter.emplace_back();
            for (int u = 0; u < h->blocks; ++u) h->inter[i].push_back(ld.unit(idx("unet.intermediate.layers.%d.conv.%d", i, u), (i || u) ? cout : cin, cout));
        }
        cin = cout;
        for (int i = 0; i < h->levels; ++i) {
            cout = cin / 2;
            Conv up;
            up.Cin = cin, up.Cout = cout, up.mode = MODE_UP;
            up.w = ld.arena.push_f16(pack_up(ld.get(idx("unet.decoder.layers.%d.conv1.0.weight", i), {cin, cout, 3, 3}), cin, cout));
            std::vector<float> sc, sh;
            ld.bn(idx("unet.decoder.layers.%d.conv1.1", i), cout, sc, sh);
            up.scale = ld.arena.push_f32(sc);
            up.shift = ld.arena.push_f32(sh);
            h->up.push_back(up);
            h->dec.emplace_back();
            for (int u = 0; u < h->blocks; ++u) h->dec[i].push_back(ld.unit(idx("unet.decoder.layers.%d.conv2.%d", i, u), u ? cout : 2 * cout, cout));
            cin = cout;
        }
        if (cin != h->base) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_create: the decoder ends with %d channels, not %d", cin, h->base);
        {
            const std::string wn = "cnn.weight";
            if (!ld.has(wn)) RVCMI_FAIL(RVCMI_ERR_MISSING, "unet_create: missing weight tensor 'cnn.weight'");
            const int hc = (int)ld.wt.find(wn)->shape[0];
            if (hc < 1 || hc > 16) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_create: a head of %d channels is not supported", hc);
            h->head.Cin = h->base, h->head.Cout = hc, h->head.mode = MODE_3X3;
            h->head.w = ld.arena.push_f16(pack_conv(ld.get(wn, {hc, h->base, 3, 3}), hc, h->base, 3));
            h->head.scale = ld.arena.push_f32(std::vector<float>(16, 1.f));
            h->head.shift = ld.arena.push_f32(padded16(ld.get("cnn.bias", {hc}), hc, 0.f));
        }
        ld.wt.require_all_used("network", {"unet.", "cnn."});  // (tensors under other prefixes belong to the rest of the f0 model)
        DeviceGuard dg(device);
        upload(h->arena, ld.arena.host);
        *out = h.release();
    });
}

int rvcmi_unet_destroy(rvcmi_unet* h) {
    return guarded([&] { delete h; });
}

int rvcmi_unet_head_channels(rvcmi_unet* h) { return h ? h->head.Cout : 0; }

size_t rvcmi_unet_workspace_bytes(rvcmi_unet* h, int B, int T) {
    size_t n = 0;
    const int rc = guarded([&] {
        if (!shape_ok(h, B, T)) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_workspace_bytes: B = %d, T = %d (T a multiple of %d)", B, T, h ? 1 << h->levels : 0);
        n = run(h, B, T, nullptr, nullptr, nullptr, nullptr, true);
    });
    return rc == RVCMI_OK ? n : 0;
}

int rvcmi_unet_forward(rvcmi_unet* h, int B, int T, const float* mel_dev, float* out_dev, void* ws_dev, void* stream) {
    return guarded([&] {
        if (!h || !mel_dev || !out_dev || !ws_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_forward: null argument");
        if (!shape_ok(h, B, T)) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_forward: B = %d, T = %d (T a multiple of %d)", B, T, 1 << h->levels);
        run(h, B, T, nullptr, nullptr, nullptr, nullptr, true);  // every grid checked before the first launch
        DeviceGuard dg(h->device);
        run(h, B, T, mel_dev, out_dev, (char*)ws_dev, (hipStream_t)stream, false);
    });
}

size_t rvcmi_unet_workspace_bytes_ragged(rvcmi_unet* h, int nseq, const int* offsets_host) {
    size_t n = 0;
    const int rc = guarded([&] {
        check_ragged(h, nseq, offsets_host, "unet_workspace_bytes_ragged");
        n = run(h, 1, offsets_host[nseq], nullptr, nullptr, nullptr, nullptr, true);  // (sizes and grids depend on the row count only)
    });
    return rc == RVCMI_OK ? n : 0;
}

int rvcmi_unet_forward_ragged(rvcmi_unet* h, int nseq, const int* offsets_host, const int* offsets_dev, const float* mel_dev, float* out_dev,
                              void* ws_dev, void* stream) {
    return guarded([&] {
        if (!h || !offsets_host || !offsets_dev || !mel_dev || !out_dev || !ws_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_forward_ragged: null argument");
        check_ragged(h, nseq, offsets_host, "unet_forward_ragged");
        const int R = offsets_host[nseq];
        run(h, 1, R, nullptr, nullptr, nullptr, nullptr, true);  // every grid checked before the first launch
        DeviceGuard dg(h->device);
        run(h, 1, R, mel_dev, out_dev, (char*)ws_dev, (hipStream_t)stream, false, offsets_dev, nseq);
    });
}

int rvcmi_unet_debug_op(int kind, int B, int H, int W, int C0, int C1, int Cout, const float* w, const float* scale, const float* shift, int relu,
                        float in_scale, float in_shift, const void* x0_dev, const void* x1_dev, const void* res_dev, void* out_dev, int ksplit,
                        int device, void* stream) {
    return guarded([&] {
        if (B < 1 || H < 1 || W < 1 || (long long)B * H * W > (1ll << 24) || !x0_dev || !out_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_debug_op: bad argument");
        DeviceGuard dg(device);
        hipStream_t st = (hipStream_t)stream;
        Ctx c;
        c.st = st;
        c.force_ksplit = ksplit;
        if (kind == 3) {  // pool
            if (C0 % 8 || H % 2 || W % 2) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_debug_op: pool shape");
            pool(c, (const _Float16*)x0_dev, (_Float16*)out_dev, B, H, W, C0);
            HIP_CHECK(hipStreamSynchronize(st));
            return;
        }
        if (!w || !scale || !shift || Cout < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_debug_op: null weights");
        Arena ar;
        Conv L;
        L.Cin = C0 + C1, L.Cout = Cout;
        const bool one = kind == 4 || kind == 5;
        if (one && (L.Cin != 1 || Cout % 8)) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_debug_op: first-layer shape");
        if (!one && (kind != 6 && Cout % 16)) RVCMI_FAIL(RVCMI_ERR_INVALID, "unet_debug_op: Cout %% 16");
        L.mode = kind == 1 || kind == 5 ? MODE_1X1 : kind == 2 ? MODE_UP : MODE_3X3;
        if (kind == 2) L.w = ar.push_f16(pack_up(w, L.Cin, Cout));
        else L.w = ar.push_f16(pack_conv(w, Cout, L.Cin, L.mode == MODE_1X1 ? 1 : 3));
        L.scale = ar.push_f32(padded16(scale, Cout, 1.f));
        L.shift = ar.push_f32(padded16(shift, Cout, 0.f));
        DevBuf wd, part;
        upload(wd, ar.host);
        c.wbase = wd.as<char>();
        if (one) {
            first(c, L, kind == 4 ? 9 : 1, (const float*)x0_dev, in_scale, in_shift, relu, (_Float16*)out_dev, B, H, W);
        } else {
            c.dry = true;
            conv(c, L, (const _Float16*)x0_dev, C0, (const _Float16*)x1_dev, C1, B, H, W, relu, (const _Float16*)res_dev, out_dev,
                 kind == 6 ? OUT_HEAD32 : OUT_NHWC16);
            c.dry = false;
            if (c.max_part) part.alloc(c.max_part);
            c.part = part.as<float>();
            conv(c, L, (const _Float16*)x0_dev, C0, (const _Float16*)x1_dev, C1, B, H, W, relu, (const _Float16*)res_dev, out_dev,
                 kind == 6 ? OUT_HEAD32 : OUT_NHWC16);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
    });
}

}  // extern "C"
