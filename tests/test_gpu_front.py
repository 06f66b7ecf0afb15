"""GPU parity of the synthesizer front (enc_p + z_p + flow^-1) and of the whole ``infer``.

Fixtures come from the REAL reference modules (oracle/make_golden.py: TextEncoder, ResidualCouplingBlock and
SynthesizerTrnMsNSFsid.infer executed on torch-CPU with seeded weights); other sizes compare against the oracle.
Bars: MFMA operands are fp16 with fp32 accumulation, fp32 LayerNorm / softmax / gates; z has unit scale, so the
bar on z is 5e-3 RMS (measured ~1e-3), and the north-star bar on the waveform stays 1e-3 RMS."""
import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden, rms
from oracle import front_oracle, nsf_oracle, synth
from oracle.front_oracle import FrontConfig

pytestmark = pytest.mark.gpu

Z_BAR = {"fp16": 5e-3, "bf16": 4e-2}
_cache = {}


def front_weights(d, in_channels=768):
    fcfg = FrontConfig(in_channels=in_channels)
    key = ("wf", in_channels, int(d["seed"]))
    if key not in _cache:
        _cache[key] = synth.make_front_weights(fcfg, int(d["seed"]))
    wf = _cache[key]
    sha = str(d["weights_sha256"]) if "weights_sha256" in d else str(d["front_sha256"])
    assert synth.weights_sha256(wf) == sha, "seeded front weights differ from the fixture's (torch RNG changed?)"
    return fcfg, wf


def hip_front(fcfg, wf, operand, gpu, max_B=2, max_T=128):
    import rvc_amd

    return rvc_amd.FrontHIP(vars(fcfg), wf, device=gpu, operand=operand, max_B=max_B, max_T=max_T)


def dev(d, k, gpu):
    return torch.from_numpy(d[k]).to(gpu)


@pytest.mark.parametrize("operand", ["fp16", "bf16"])
@pytest.mark.parametrize("name", golden_names("front_"))
def test_front_matches_reference_golden(name, operand, gpu):
    d = load_golden(name)
    fcfg, wf = front_weights(d, int(d["in_channels"]))
    fr = hip_front(fcfg, wf, operand, gpu)
    fh = max(int(d["flow_head"]), 0)
    args = (dev(d, "phone", gpu), dev(d, "pitch", gpu), dev(d, "lengths", gpu), dev(d, "g", gpu))
    nz = dev(d, "noise", gpu)
    z = fr(*args, fh, noise=nz).cpu()
    assert z.shape == d["z"].shape and torch.isfinite(z).all()
    e = rms(z, d["z"])
    assert e <= Z_BAR[operand], "%s/%s: z RMS error %.3e exceeds %.1e" % (name, operand, e, Z_BAR[operand])
    if operand == "fp16":  # stage-by-stage (channels-last taps): localises a regression
        for tap, bar in (("emb", 2e-3), ("attn0", 4e-3), ("layer0", 4e-3), ("layer5", 5e-3), ("z_p", 5e-3)):
            ref = d[tap]
            got = fr.debug_tap(tap, *args, fh, noise=nz)
            assert got.shape == ref.shape, (tap, got.shape, ref.shape)
            et = rms(got, ref)
            assert et <= bar, "%s: tap %s RMS error %.3e exceeds %.1e" % (name, tap, et, bar)


def test_padding_rows_do_not_leak(gpu):
    """Rows beyond phone_lengths are masked exactly as x_mask does (encoders.py:145-148, attentions.py:114-115):
    the valid part of z must not depend on what the padding rows contain."""
    d = load_golden("front_v2_B2_T50")
    fcfg, wf = front_weights(d)
    fr = hip_front(fcfg, wf, "fp16", gpu)
    phone = dev(d, "phone", gpu).clone()
    args = lambda ph: (ph, dev(d, "pitch", gpu), dev(d, "lengths", gpu), dev(d, "g", gpu))
    nz = dev(d, "noise", gpu)
    z0 = fr(*args(phone), 0, noise=nz).cpu()
    L1 = int(d["lengths"][1])
    phone[1, L1:] = 37.0  # garbage in the padded frames of utterance 1
    z1 = fr(*args(phone), 0, noise=nz).cpu()
    assert torch.equal(z0[0], z1[0])
    assert torch.equal(z0[1, :, :L1], z1[1, :, :L1])
    assert (z1[1, :, L1:] == 0).all()


@pytest.mark.parametrize("T,B,fh", [(1, 1, 0), (31, 1, 0), (64, 2, 0), (65, 1, 0), (200, 1, 30)])
def test_front_against_oracle_other_sizes(T, B, fh, gpu):
    fcfg = FrontConfig()
    wf = synth.make_front_weights(fcfg, 77)
    fr = hip_front(fcfg, wf, "fp16", gpu, max_B=2, max_T=256)
    phone = synth.make_phone(B, T, 768, 77)
    pitch = synth.make_pitch(synth.make_f0(B, T))
    lengths = torch.tensor([T, max(1, T - 9)][:B])
    sid = torch.tensor([1, 7][:B])
    gen = torch.Generator().manual_seed(3)
    noise = torch.randn(B, 192, T - fh, generator=gen)
    with torch.no_grad():
        z, m1, g = front_oracle.infer_front(fcfg, wf, phone, pitch, lengths, sid, noise, fh if fh else None)
        z = z * m1
    got = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), fh, noise=noise.to(gpu)).cpu()
    e = rms(got, z)
    assert e <= Z_BAR["fp16"], "T=%d B=%d: z RMS error %.3e" % (T, B, e)


class _Net:
    """What infer_hip needs of net_g: emb_g and dec (no reference import on the GPU box)."""

    def __init__(self, wf, dec):
        self.emb_g = lambda sid: wf["emb_g.weight"].to(sid.device)[sid]
        self.dec = dec


@pytest.mark.parametrize("name", golden_names("infer_full_"))
def test_whole_infer_matches_reference_golden(name, gpu):
    """enc_p -> z_p -> flow^-1 -> NSF generator, all HIP, against the reference's net_g.infer waveform (<= 1e-3 RMS)."""
    import rvc_amd

    infer_hip = rvc_amd.infer_hip

    d = load_golden(name)
    fcfg, wf = front_weights(d)
    cfg = nsf_oracle.CONFIGS["v2_48k"]
    wd = synth.make_dec_weights(cfg, int(d["seed"]))
    assert synth.weights_sha256(wd) == str(d["dec_sha256"])
    fr = hip_front(fcfg, wf, "fp16", gpu, max_B=1, max_T=128)
    dec = rvc_amd.NSFGeneratorHIP(vars(cfg), wd, device=gpu, operand="fp16", max_B=1, max_T=128)
    T = d["phone"].shape[1]
    opt = lambda k: None if int(d[k]) < 0 else int(d[k])
    out = infer_hip(_Net(wf, dec), fr, dev(d, "phone", gpu), torch.tensor([T], device=gpu), dev(d, "sid", gpu), dev(d, "pitch", gpu),
                    dev(d, "pitchf", gpu), opt("skip_head"), opt("return_length"), opt("return_length2"),
                    noise_zp=dev(d, "noise_zp", gpu), noise_dec=dev(d, "noise_dec", gpu)).cpu()
    assert out.shape == d["out"].shape
    e = rms(out, d["out"])
    assert e <= 1e-3, "%s: waveform RMS error %.3e vs the reference infer exceeds 1e-3" % (name, e)


def test_front_rng_stream_matches_reference_draw(gpu):
    """Without noise= the front draws randn_like(m_p) once, [B, inter, T - flow_head], from the input's device generator."""
    fcfg = FrontConfig()
    wf = synth.make_front_weights(fcfg, 5)
    fr = hip_front(fcfg, wf, "fp16", gpu, max_B=1, max_T=64)
    T = 40
    phone = synth.make_phone(1, T, 768, 5).to(gpu)
    pitch = synth.make_pitch(synth.make_f0(1, T)).to(gpu)
    g = wf["emb_g.weight"][:1].to(gpu)
    torch.manual_seed(11)
    a = fr(phone, pitch, None, g, 4)
    after = torch.rand(1, device=gpu)
    torch.manual_seed(11)
    nz = torch.randn(1, 192, T - 4, device=gpu)
    b = fr(phone, pitch, None, g, 4, noise=nz)
    assert torch.equal(a, b) and torch.equal(after, torch.rand(1, device=gpu))


def test_front_rejects_bad_input(gpu):
    import rvc_amd

    fcfg = FrontConfig()
    wf = synth.make_front_weights(fcfg, 5)
    fr = hip_front(fcfg, wf, "fp16", gpu, max_B=1, max_T=32)
    with pytest.raises(ValueError):
        fr(torch.zeros(1, 8, 100, device=gpu), None, None, None)
    with pytest.raises(ValueError):
        rvc_amd.FrontHIP(vars(fcfg), wf, device=gpu, operand="fp32")
    bad = dict(wf)
    del bad["flow.flows.2.post.bias"]
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.FrontHIP(vars(fcfg), bad, device=gpu)
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.FrontHIP(vars(FrontConfig(n_heads=4)), wf, device=gpu)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_wn_layer_forms_agree(mode, gpu):
    """One WN layer exists in three forms (option FR_WN_SPLIT): 0 = k_fr_wn (one launch), 1 = gate + res_skip launches with the channel pairs
    split over 3x the blocks (bit-identical to 0: same K loops, same epilogue order), 2 = the gate with the TAPS split over the waves (the
    default for small grids; another summation order).  Every form against the reference goldens; 1 bit-equal to 0."""
    for name in ("front_v2_B2_T50", "front_v2_B1_T100_head6"):
        d = load_golden(name)
        fcfg, wf = front_weights(d, int(d["in_channels"]))
        fr = hip_front(fcfg, wf, "fp16", gpu)
        fh = max(int(d["flow_head"]), 0)
        args = (dev(d, "phone", gpu), dev(d, "pitch", gpu), dev(d, "lengths", gpu), dev(d, "g", gpu))
        fr.set_option("FR_WN_SPLIT", mode)
        z = fr(*args, fh, noise=dev(d, "noise", gpu))
        e = rms(z.cpu(), d["z"])
        assert e <= Z_BAR["fp16"], "%s (FR_WN_SPLIT=%d): z RMS error %.3e" % (name, mode, e)
        fr.set_option("FR_WN_SPLIT", 0)
        z0 = fr(*args, fh, noise=dev(d, "noise", gpu))
        if mode == 1:
            assert torch.equal(z, z0)
        else:
            assert rms(z.cpu(), z0.cpu()) <= 2e-3


@pytest.mark.parametrize("ks", [3, 7])
def test_wn_gate_tap_split_with_other_flow_kernel_sizes(ks, gpu):
    """The tap-split gate launches 64 x flow_kernel_size threads (wave w = tap w); every shipped config has 5 taps, other odd sizes take the
    generic staging helper: the front with flow_kernel_size 3 / 7 against the oracle, in the one-launch form and in the tap-split form."""
    fcfg = FrontConfig(flow_kernel_size=ks)
    wf = synth.make_front_weights(fcfg, 21)
    T, B = 90, 2
    phone = synth.make_phone(B, T, 768, 21)
    pitch = synth.make_pitch(synth.make_f0(B, T))
    lengths, sid = torch.tensor([T, T - 23]), torch.tensor([3, 5])
    noise = torch.randn(B, 192, T, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        z, m1, g = front_oracle.infer_front(fcfg, wf, phone, pitch, lengths, sid, noise)
        z = z * m1
    fr = hip_front(fcfg, wf, "fp16", gpu, max_B=B, max_T=128)
    for mode in (0, 2):
        fr.set_option("FR_WN_SPLIT", mode)
        got = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), 0, noise=noise.to(gpu)).cpu()
        e = rms(got, z)
        assert e <= Z_BAR["fp16"], "flow_kernel_size %d, FR_WN_SPLIT=%d: z RMS error %.3e" % (ks, mode, e)


@pytest.mark.parametrize("fused_ffn", [True, False, "split", "split_nj1"])
def test_front_large_batch_tile_height_and_unfused_ffn(fused_ffn, gpu):
    """Large batches run 64-row time tiles (pick_nj) and the FFN exists in three forms -- one fused launch (k_fr_ffn, large
    grids), two plain conv launches, and the split form for small grids (k_fr_ffn_part: hidden channels over 4x the blocks +
    k_fr_ffn_ln) -- : force every code path on a small golden input through the handle's test options."""
    for name in ("front_v2_B2_T50", "front_v2_B1_T100_head6"):
        d = load_golden(name)
        fcfg, wf = front_weights(d, int(d["in_channels"]))
        fr = hip_front(fcfg, wf, "fp16", gpu)
        fr.set_option("FR_NJ", 1 if fused_ffn == "split_nj1" else 2)
        fr.set_option("FR_FFN_SPLIT", 1 if str(fused_ffn).startswith("split") else 0)
        if fused_ffn is False:
            fr.set_option("FR_NO_FFN_FUSION", 1)
        fh = max(int(d["flow_head"]), 0)
        z = fr(dev(d, "phone", gpu), dev(d, "pitch", gpu), dev(d, "lengths", gpu), dev(d, "g", gpu), fh, noise=dev(d, "noise", gpu)).cpu()
        e = rms(z, d["z"])
        assert e <= Z_BAR["fp16"], "%s (NJ=2, fused_ffn=%s): z RMS error %.3e" % (name, fused_ffn, e)


def test_front_full_clip_size_vs_oracle_and_windowed_waveform(gpu):
    """BASELINE size (T = 1198 frames = one 10 s clip): the front against its oracle over the whole clip (the attention is
    global, so no windowing is possible for it), then the whole infer's waveform against the oracle generator on a
    380-frame window fed with the HIP front's own z (the decoder is local; its CPU oracle needs ~1 s per 380 frames)."""
    import rvc_amd

    T = 1198
    fcfg = FrontConfig()
    wf = synth.make_front_weights(fcfg, 1234)
    cfg = nsf_oracle.CONFIGS["v2_48k"]
    wd = synth.make_dec_weights(cfg, 1234)
    phone = synth.make_phone(1, T, 768, 1234)
    pitchf = synth.make_f0(1, T)
    pitch = synth.make_pitch(pitchf)
    lengths, sid = torch.tensor([T]), torch.tensor([0])
    nz = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        zr, m1, g = front_oracle.infer_front(fcfg, wf, phone, pitch, lengths, sid, nz)
    fr = hip_front(fcfg, wf, "fp16", gpu, max_B=1, max_T=T)
    z = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), 0, noise=nz.to(gpu))
    e = rms(z.cpu(), zr * m1)
    assert e <= Z_BAR["fp16"], "full-size front: z RMS error %.3e" % e
    dec = rvc_amd.NSFGeneratorHIP(vars(cfg), wd, device=gpu, operand="fp16", max_B=1, max_T=T)
    noise = nsf_oracle.reference_noise(1, T, cfg.upp, 114514)
    f0u = torch.zeros_like(pitchf)  # unvoiced: no phase history, so a window of the clip is exactly comparable
    out = dec(z, f0u.to(gpu), g.to(gpu), noise=noise.to(gpu)).cpu()
    a, b, m = 500, 800, 40
    with torch.no_grad():
        ref = nsf_oracle.generator_forward(cfg, wd, (zr * m1)[:, :, a - m:b + m], f0u[:, a - m:b + m], g,
                                           noise[:, (a - m) * cfg.upp:(b + m) * cfg.upp])
    x = out[0, 0, a * cfg.upp:b * cfg.upp]
    y = ref[0, 0, m * cfg.upp:(m + b - a) * cfg.upp]
    ew = rms(x, y)
    assert ew <= 1e-3, "full-size whole infer (window %d..%d): waveform RMS error %.3e" % (a, b, ew)


def test_whole_infer_full_clip_voiced_vs_oracle(gpu):
    """BASELINE configs[1] end to end: the whole ``infer`` (front + generator on HIP) over one 10 s clip with VOICED pitch
    (80 % of the 1198 frames) against oracle front + oracle generator -- the complete waveform, no window."""
    import rvc_amd

    T = 1198
    fcfg, cfg = FrontConfig(), nsf_oracle.CONFIGS["v2_48k"]
    wf, wd = synth.make_front_weights(fcfg, 1234), synth.make_dec_weights(cfg, 1234)
    phone, pitchf = synth.make_phone(1, T, 768, 1234), synth.make_f0(1, T)
    pitch = synth.make_pitch(pitchf)
    assert float((pitchf > 0).float().mean()) > 0.5
    lengths, sid = torch.tensor([T]), torch.tensor([0])
    nz = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(8))
    noise = nsf_oracle.reference_noise(1, T, cfg.upp, 114514)
    with torch.no_grad():
        zr, m1, g = front_oracle.infer_front(fcfg, wf, phone, pitch, lengths, sid, nz)
        ref = nsf_oracle.generator_forward(cfg, wd, zr * m1, pitchf, g, noise)
    fr = hip_front(fcfg, wf, "fp16", gpu, max_B=1, max_T=T)
    dec = rvc_amd.NSFGeneratorHIP(vars(cfg), wd, device=gpu, operand="fp16", max_B=1, max_T=T)
    z = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), 0, noise=nz.to(gpu))
    out = dec(z, pitchf.to(gpu), g.to(gpu), noise=noise.to(gpu)).cpu()
    e = rms(out, ref)
    assert e <= 1e-3, "whole infer, full voiced clip: waveform RMS error %.3e" % e


def test_front_batch_16_equals_single_clips(gpu):
    """The large-batch launch shapes of the front (64-row tiles, pick_nj) at B = 16, T = 1198 with ragged lengths: every item
    must equal the same clip run alone (tile height changes no element's summation order)."""
    B, T = 16, 1198
    fcfg = FrontConfig()
    wf = synth.make_front_weights(fcfg, 1234)
    phone, pitchf = synth.make_phone(B, T, 768, 1234), synth.make_f0(B, T)
    pitch = synth.make_pitch(pitchf)
    lengths = torch.tensor([T - 31 * b for b in range(B)])
    sid = torch.arange(B) % 7
    nz = torch.randn(B, 192, T, generator=torch.Generator().manual_seed(8))
    g = wf["emb_g.weight"][sid].unsqueeze(-1)
    fr = hip_front(fcfg, wf, "fp16", gpu, max_B=B, max_T=T)
    # (the FFN form pinned: a single clip would otherwise take the split form, whose partial sums add in another order; the same for the
    #  tap-split gate of the WN layers, round 6)
    fr.set_option("FR_FFN_SPLIT", 0)
    fr.set_option("FR_WN_SPLIT", 0)
    z = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), 0, noise=nz.to(gpu))
    assert z.shape == (B, 192, T) and torch.isfinite(z).all()
    for b in (0, 5, 15):
        one = fr(phone[b:b + 1].to(gpu), pitch[b:b + 1].to(gpu), lengths[b:b + 1].to(gpu), g[b:b + 1].to(gpu), 0, noise=nz[b:b + 1].to(gpu))
        e = rms(one[0].cpu(), z[b].cpu())
        assert e <= 1e-6, "front batch item %d differs from its single-clip result: %.3e" % (b, e)
        if int(lengths[b]) < T:
            assert float(z[b, :, int(lengths[b]):].abs().max()) == 0.0  # masked tail
    fr.set_option("FR_FFN_SPLIT", None)   # the launcher's own choice for one clip (split): same z to operand rounding
    fr.set_option("FR_WN_SPLIT", None)
    one = fr(phone[5:6].to(gpu), pitch[5:6].to(gpu), lengths[5:6].to(gpu), g[5:6].to(gpu), 0, noise=nz[5:6].to(gpu))
    assert rms(one[0].cpu(), z[5].cpu()) <= 2e-3
    with torch.no_grad():
        zr, m1, _ = front_oracle.infer_front(fcfg, wf, phone[15:16], pitch[15:16], lengths[15:16], sid[15:16], nz[15:16])
    assert rms(z[15:16].cpu(), zr * m1) <= Z_BAR["fp16"]


def _f0_with_voiced_fraction(T, frac):
    """synth.make_f0's contour (220 * 2^sin(2 pi t / 300) Hz) with the first (1 - frac) of every 200 frames unvoiced."""
    f0 = synth.make_f0(1, T).clone()
    t = torch.arange(T)
    f0[0] = 220.0 * torch.pow(2.0, torch.sin(2 * np.pi * t.float() / 300.0))
    f0[0, (t % 200) < int(round(200 * (1.0 - frac)))] = 0.0
    return f0


def _scale_z_path(wd, gain):
    """`gain` on the decoder's z path: conv_pre and cond (weights and biases) x gain.  The leaky-ReLU stack is positively homogeneous
    up to the 0.1-sized biases, so the stage activations -- and the pre-tanh waveform -- scale with it, while the excitation path
    (noise_convs on the harmonic source) keeps its amplitude: gain 0.5 = source-dominated, small waveform; gain 2 = z-dominated, tanh
    driven harder.  (A gain on every conv instead would compound over 76 layers.)"""
    w = dict(wd)
    for k in ("conv_pre.weight", "conv_pre.bias", "cond.weight", "cond.bias"):
        w[k] = wd[k] * gain
    return w


def test_whole_infer_parity_sweep_over_weight_draws_gains_and_voicing(gpu, capsys):
    """The parity headroom of the shipped arithmetic (fp16 MFMA operands + fp16 inter-stage streams) is not a property of ONE weight
    draw: whole ``infer`` (rvc/layers/synthesizers.py:160-203) on a full 10 s clip, T = 1198, against the oracle (pinned to the reference
    at 2e-6 by the goldens) for 5 weight seeds x z-path gains {0.5, 1, 2} x voiced fractions {0.2, 0.8} -- 30 clips.  Every one must
    meet the north star's 1e-3 RMS; the worst is printed."""
    import rvc_amd

    T = 1198
    fcfg, cfg = FrontConfig(), nsf_oracle.CONFIGS["v2_48k"]
    torch.set_num_threads(min(32, torch.get_num_threads() if torch.get_num_threads() > 8 else 16))
    rows = []
    for seed in (1234, 7, 99, 2024, 31337):
        wf, wd0 = synth.make_front_weights(fcfg, seed), synth.make_dec_weights(cfg, seed)
        fr = hip_front(fcfg, wf, "fp16", gpu, max_B=1, max_T=T)
        phone = synth.make_phone(1, T, 768, seed)
        lengths, sid = torch.tensor([T]), torch.tensor([seed % 100])
        nz = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(seed + 8))
        noise = nsf_oracle.reference_noise(1, T, cfg.upp, 114514 + seed)
        for frac in (0.2, 0.8):
            pitchf = _f0_with_voiced_fraction(T, frac)
            pitch = synth.make_pitch(pitchf)
            with torch.no_grad():
                zr, m1, g = front_oracle.infer_front(fcfg, wf, phone, pitch, lengths, sid, nz)
            z = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), 0, noise=nz.to(gpu))
            for gain in (0.5, 1.0, 2.0):
                wd = _scale_z_path(wd0, gain)
                with torch.no_grad():
                    ref = nsf_oracle.generator_forward(cfg, wd, zr * m1, pitchf, g, noise)
                dec = rvc_amd.NSFGeneratorHIP(vars(cfg), wd, device=gpu, operand="fp16", max_B=1, max_T=T)
                out = dec(z, pitchf.to(gpu), g.to(gpu), noise=noise.to(gpu)).cpu()
                del dec
                assert torch.isfinite(out).all()
                rows.append((rms(out, ref), seed, gain, frac, float(ref.pow(2).mean().sqrt()), float((ref.abs() > 0.99).float().mean())))
    rows.sort(reverse=True)
    with capsys.disabled():
        print("\n[whole-infer parity sweep, T=1198, fp16 operands + fp16 streams] %d clips: worst RMS %.3e, median %.3e, best %.3e; the five worst:"
              % (len(rows), rows[0][0], rows[len(rows) // 2][0], rows[-1][0]))
        for r in rows[:5]:
            print("    rms %.3e  seed %-6d gain %.1f voiced %.1f  waveform rms %.3f  beyond +-0.99: %.4f" % r)
    assert rows[0][0] <= 1e-3, "whole infer parity sweep: worst RMS %.3e (seed %d, gain %.1f, voiced fraction %.1f)" % rows[0][:4]


def _scale_homogeneously(wd, G):
    """The SAME function with every activation of the stack G times larger: the leaky-ReLU stack is positively homogeneous, so scaling
    what enters it (conv_pre, cond, the noise convs: weights and biases) and every bias inside it (ups, ResBlock convs) by G and
    conv_post by 1 / G changes nothing in exact arithmetic -- and with G a power of two nothing in fp32 either."""
    w = {}
    for k, v in wd.items():
        if k.startswith(("conv_pre.", "cond.", "noise_convs.")) or (k.endswith(".bias") and k.startswith(("ups.", "resblocks."))):
            w[k] = v * G
        elif k == "conv_post.weight":
            w[k] = v / G
        else:
            w[k] = v
    return w


def test_fp16_range_headroom_and_saturation_against_the_fp32_reference(gpu, capsys):
    """fp16 MFMA operands and fp16 inter-stage streams have a RANGE (+-65504) as well as a precision.  The generator is rescaled
    homogeneously (`_scale_homogeneously`: same function, bit-identical fp32 reference for a power-of-two G, every activation G x larger):

      * G puts the largest tapped activation at ~1/8 of the fp16 range: the error against the reference must be the unscaled run's
        (within 10 %) -- the parity claim does not depend on the absolute scale of a checkpoint's activations;
      * G puts it 1.25-2.5x BEYOND the range (asserted on the oracle's fp32 taps): the publish path converts with SATURATION
        (`v_med3_f32(x, 0.1 x, 65504)` in pack4_lrelu, `pack4_h` for the streams; csrc/mfma_conv.hpp), so the clipped peaks cost accuracy
        locally but the waveform stays finite and close to the fp32 reference; an overflowing conversion would produce inf, and inf - inf =
        NaN in the next conv."""
    import rvc_amd

    T = 200
    cfg = nsf_oracle.CONFIGS["v2_48k"]
    wd = synth.make_dec_weights(cfg, 1234)
    z, f0, g = synth.make_dec_inputs(cfg, 1, T)
    noise = nsf_oracle.reference_noise(1, T, cfg.upp)
    taps = {}
    with torch.no_grad():
        ref = nsf_oracle.generator_forward(cfg, wd, z, f0, g, noise, taps=taps)
    amax = max(float(v.abs().max()) for k, v in taps.items() if k != "har")
    run = lambda w: rvc_amd.NSFGeneratorHIP(vars(cfg), w, device=gpu, operand="fp16", max_B=1, max_T=T)(
        z.to(gpu), f0.to(gpu), g.to(gpu), noise=noise.to(gpu)).cpu()
    out0 = run(wd)
    e0 = rms(out0, ref)
    G_in = 2.0 ** np.floor(np.log2(65504.0 / 8 / amax))
    G_sat = 2.0 ** np.ceil(np.log2(1.25 * 65504.0 / amax))
    res = {}
    for name, G in (("inside", G_in), ("beyond", G_sat)):
        w = _scale_homogeneously(wd, G)
        tp = {}
        with torch.no_grad():
            r = nsf_oracle.generator_forward(cfg, w, z, f0, g, noise, taps=tp)
        assert torch.equal(r, ref), "the rescaled fp32 reference must be bit-identical (G = %g)" % G
        peak = max(float(v.abs().max()) for k, v in tp.items() if k != "har")
        frac = float(np.mean([float((v.abs() > 65504).float().mean()) for k, v in tp.items() if k != "har"]))
        o = run(w)
        assert torch.isfinite(o).all(), "%s the fp16 range (G = %g): non-finite waveform" % (name, G)
        res[name] = (G, peak, frac, rms(o, ref), rms(o, out0))
    with capsys.disabled():
        print("\n[fp16 range] unscaled: largest tapped activation %.1f, RMS vs the reference %.3e" % (amax, e0))
        for name in ("inside", "beyond"):
            print("    %s: G = 2^%d, largest tapped activation %.3g (%.2f x 65504), %.4f %% of the tapped values beyond the range; "
                  "RMS vs the fp32 reference %.3e, vs the unscaled HIP run %.3e" % ((name, int(np.log2(res[name][0])), res[name][1],
                                                                                   res[name][1] / 65504.0, 100 * res[name][2]) + res[name][3:]))
    # (the rescaled run is NOT bit-similar to the unscaled one although fp32 mode is, tools/diag_scale.py: fp16-subnormal weights differ
    #  in the last bit, and every later fp16 quantisation amplifies ulp-level differences -- two equally valid rounding paths end up
    #  ~2e-4 apart, as far as each is from the reference; what must hold is that the ERROR does not depend on the scale)
    assert res["inside"][1] < 65504 / 4 and res["inside"][3] <= 1e-3 and abs(res["inside"][3] - e0) <= 0.1 * e0, (res["inside"], e0)
    assert res["beyond"][1] > 65504, "the case must drive activations beyond the fp16 range (peak %.3g)" % res["beyond"][1]
    assert res["beyond"][3] <= 5e-2, "saturating conversions: RMS %.3e vs the fp32 reference with %.4f %% of the activations clipped" % (
        res["beyond"][3], 100 * res["beyond"][2])
