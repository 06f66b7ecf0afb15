// What was left of the RMVPE f0 network (rvc/f0/rmvpe.py) next to gru.hip and unet.hip, for gfx950 -- like them BEYOND the scope table
// (SURVEY.md section 8): the log-mel front end (rvc/f0/mel.py:58-71 over rvc/f0/stft.py:165-180, keyshift 0, speed 1, center=True) that
// turns a waveform into the U-Net's input, and the Linear(512, 360) + sigmoid (rvc/f0/e2e.py:33-35) behind the GRU.  Kernels in
// rmvpe_kernels.hpp.  With them a caller of the C ABI computes f0 from a waveform without torch:
//   rvcmi_mel_forward -> rvcmi_unet_forward -> rvcmi_gru_forward -> rvcmi_rmvpe_head -> rvcmi_glue_rmvpe_f0_key.
#include <cmath>
#include <memory>

#include "common.hpp"
#include "rmvpe_kernels.hpp"

using namespace rvcmi;

struct rvcmi_mel {
    int device = 0, n_fft = 0, hop = 0;
    float clamp = 0.f;
    DevBuf window, tw, basisT, band;
};

extern "C" {

int rvcmi_mel_create(int n_fft, int hop, int win_length, int n_mels, const float* mel_basis, float clamp, int device, rvcmi_mel** out) {
    return guarded([&] {
        if (!mel_basis || !out) RVCMI_FAIL(RVCMI_ERR_INVALID, "mel_create: null argument");
        if (n_fft != MEL_NFFT || win_length != n_fft || n_mels != MEL_NMELS || hop < 1 || !(clamp > 0.f))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "mel_create: n_fft %d / win_length %d / n_mels %d / hop %d / clamp %g not supported (1024, 1024, 128, >= 1, > 0)",
                       n_fft, win_length, n_mels, hop, (double)clamp);
        DeviceGuard dg(device);
        std::unique_ptr<rvcmi_mel> h(new rvcmi_mel());
        h->device = device;
        h->n_fft = n_fft;
        h->hop = hop;
        h->clamp = clamp;
        const double pi = 3.14159265358979323846;
        std::vector<double> win(MEL_NFFT), tw(2 * MEL_NFFT);
        for (int i = 0; i < MEL_NFFT; ++i) {
            win[i] = 0.5 - 0.5 * std::cos(2.0 * pi * i / MEL_NFFT);  // torch.hann_window(win_length): periodic
            tw[2 * i] = std::cos(2.0 * pi * i / MEL_NFFT);
            tw[2 * i + 1] = -std::sin(2.0 * pi * i / MEL_NFFT);
        }
        // the filter bank transposed to [bin][mel], and per mel row the band [first non-zero, last non-zero + 1) of the dense matrix: a sum over
        // it equals the sum over the whole row for ANY matrix (a row without structure simply has the band [0, 513); an all-zero row [0, 0))
        std::vector<float> bt((size_t)MEL_BINS * MEL_NMELS);
        std::vector<int> band(2 * MEL_NMELS);
        for (int m = 0; m < MEL_NMELS; ++m) {
            int lo = MEL_BINS, hi = 0;
            for (int k = 0; k < MEL_BINS; ++k) {
                const float v = mel_basis[(size_t)m * MEL_BINS + k];
                bt[(size_t)k * MEL_NMELS + m] = v;
                if (v != 0.f) {  // (a NaN is not equal to 0 either: it stays inside the band and reaches the result)
                    lo = std::min(lo, k);
                    hi = k + 1;
                }
            }
            band[2 * m] = hi ? lo : 0;
            band[2 * m + 1] = hi;
        }
        upload(h->window, win);
        upload(h->tw, tw);
        upload(h->basisT, bt);
        upload(h->band, band);
        *out = h.release();
    });
}

int rvcmi_mel_destroy(rvcmi_mel* h) {
    return guarded([&] { delete h; });
}

int64_t rvcmi_mel_frames(rvcmi_mel* h, int64_t n) {
    if (!h || n <= h->n_fft / 2) return 0;
    return n / h->hop + 1;
}

int rvcmi_mel_forward(rvcmi_mel* h, int B, int64_t n, const float* wav, int round_half, int T_pad, float* out, void* stream) {
    return guarded([&] {
        if (!h || !wav || !out) RVCMI_FAIL(RVCMI_ERR_INVALID, "mel_forward: null argument");
        const int64_t T = rvcmi_mel_frames(h, n);
        if (T < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "mel_forward: n = %lld is not longer than the reflection pad %d", (long long)n, h->n_fft / 2);
        if (B < 1 || B > 65535 || T > (1ll << 30) || T_pad < T || n > (1ll << 40))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "mel_forward: B = %d, %lld frames, T_pad = %d", B, (long long)T, T_pad);
        DeviceGuard dg(h->device);
        hipLaunchKernelGGL(k_rmvpe_logmel, dim3((unsigned)((T_pad + MEL_FT - 1) / MEL_FT), (unsigned)B), dim3(256), 0, (hipStream_t)stream, wav, n,
                           h->hop, (int)T, T_pad, h->window.as<double>(), h->tw.as<double2>(), h->basisT.as<float>(), h->band.as<int2>(), h->clamp,
                           round_half ? 1 : 0, out);
        HIP_CHECK(hipGetLastError());
    });
}

int rvcmi_rmvpe_head(const float* y, int M, const float* w, const float* b, int half_operands, float* salience, void* stream) {
    return guarded([&] {
        if (!y || !w || !b || !salience || M < 1 || M > (1 << 30)) RVCMI_FAIL(RVCMI_ERR_INVALID, "rmvpe_head: bad argument");
        const dim3 grid((unsigned)((M + 31) / 32), (HEAD_N + 127) / 128);
        if (half_operands)
            hipLaunchKernelGGL(k_rmvpe_head<true>, grid, dim3(256), 0, (hipStream_t)stream, y, w, b, salience, M);
        else
            hipLaunchKernelGGL(k_rmvpe_head<false>, grid, dim3(256), 0, (hipStream_t)stream, y, w, b, salience, M);
        HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
