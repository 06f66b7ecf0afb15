"""GPU tests of the front's ``"fp16x2"`` operand mode (csrc/front_split_kernels.hpp): every MFMA operand a (hi, lo') pair of fp16 values,
fp32-grade enc_p / flow on the fp16 matrix cores.

The yardstick is the CPU emulator of the same arithmetic (tests/front_split_cases.py).  Bars: 4 x the emulator's own error on the same
inputs against the same reference -- the margin is for what the emulator does not reproduce (accumulation order, the hardware exp of
softmax / sigmoid / tanh); it was set before anything ran on a GPU.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import front_split_cases as fs
from conftest import load_golden, rms
from oracle import nsf_oracle, synth
from oracle.front_oracle import FrontConfig
from test_gpu_dropin import make_cpt, rvc_tree  # noqa: F401  (the skeleton RVC checkout of the drop-in tests)

pytestmark = pytest.mark.gpu

GOLDENS = ("front_v1_B1_T40", "front_v2_B2_T50", "front_v2_B1_T100_head6")
TAPS = ("emb", "attn0", "layer0", "layer5", "z_p")
MARGIN = 4.0
_cache = {}


def golden_case(name):
    """The fixture, its seeded weights and the EMULATOR's error against it (z and every tap), computed once."""
    if name not in _cache:
        d = load_golden(name)
        fcfg = FrontConfig(in_channels=int(d["in_channels"]))
        wf = synth.make_front_weights(fcfg, int(d["seed"]))
        assert synth.weights_sha256(wf) == str(d["weights_sha256"]), "seeded front weights differ from the fixture's"
        taps = {}
        z = fs.run_front("fp16x2", fcfg, wf, *(torch.from_numpy(d[k]) for k in ("phone", "pitch", "lengths", "sid", "noise")),
                         max(int(d["flow_head"]), 0), taps)
        emu = {"z": rms(z, d["z"])}
        emu.update({t: rms(taps[t], d[t]) for t in TAPS})
        _cache[name] = (d, fcfg, wf, emu)
    return _cache[name]


def hip_front(fcfg, wf, gpu, operand="fp16x2", max_B=2, max_T=128):
    import rvc_amd

    return rvc_amd.FrontHIP(vars(fcfg), wf, device=gpu, operand=operand, max_B=max_B, max_T=max_T)


def dev(d, k, gpu):
    return torch.from_numpy(d[k]).to(gpu)


def golden_args(d, gpu):
    return (dev(d, "phone", gpu), dev(d, "pitch", gpu), dev(d, "lengths", gpu), dev(d, "g", gpu)), max(int(d["flow_head"]), 0), dev(d, "noise", gpu)


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_z_and_taps_within_4x_the_emulator(name, gpu):
    d, fcfg, wf, emu = golden_case(name)
    fr = hip_front(fcfg, wf, gpu)
    args, fh, nz = golden_args(d, gpu)
    z = fr(*args, fh, noise=nz).cpu()
    assert z.shape == d["z"].shape and torch.isfinite(z).all()
    got = {"z": rms(z, d["z"])}
    for tap in TAPS:
        t = fr.debug_tap(tap, *args, fh, noise=nz)
        assert t.shape == d[tap].shape, (tap, t.shape, d[tap].shape)
        got[tap] = rms(t, d[tap])
    print("\n[%s] RMS against the golden, GPU / emulator: " % name + ", ".join("%s %.3e / %.3e" % (k, got[k], emu[k]) for k in got))
    for k in got:
        assert got[k] <= MARGIN * emu[k], "%s: %s RMS %.3e exceeds %g x the emulator's %.3e" % (name, k, got[k], MARGIN, emu[k])


def oracle_case(T, B, fh, seed=77):
    key = ("oracle", T, B, fh)
    if key not in _cache:
        fcfg = FrontConfig()
        wf = synth.make_front_weights(fcfg, seed)
        phone = synth.make_phone(B, T, 768, seed)
        pitch = synth.make_pitch(synth.make_f0(B, T))
        lengths = torch.tensor([T, max(1, T - 9)][:B])  # B = 2: ragged
        sid = torch.tensor([1, 7][:B])
        noise = torch.randn(B, 192, T - fh, generator=torch.Generator().manual_seed(3))
        a = (fcfg, wf, phone, pitch, lengths, sid, noise, fh)
        emu = fs.run_front("fp16x2", *a)
        z64 = fs.run_front("fp32", *a, dtype=torch.float64)
        _cache[key] = (fcfg, wf, phone, pitch, lengths, wf["emb_g.weight"][sid].unsqueeze(-1), noise, emu, rms(emu, z64))
    return _cache[key]


@pytest.mark.parametrize("T,B,fh", [(1, 1, 0), (31, 1, 0), (33, 2, 0), (65, 1, 0), (70, 1, 6)])
def test_tile_edges_against_the_emulator(T, B, fh, gpu):
    """The time tile is 32 rows.  The GPU against the emulator, within 4 x the emulator's own error against the fp64 oracle."""
    fcfg, wf, phone, pitch, lengths, g, noise, emu, e_emu = oracle_case(T, B, fh)
    fr = hip_front(fcfg, wf, gpu)
    z = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), fh, noise=noise.to(gpu)).cpu()
    e = rms(z, emu)
    print("\n[T=%d B=%d flow_head=%d] GPU against the emulator %.3e; the emulator against the fp64 oracle %.3e" % (T, B, fh, e, e_emu))
    assert z.shape == emu.shape and torch.isfinite(z).all()
    assert e <= MARGIN * e_emu, "T=%d B=%d: GPU differs from the emulator by %.3e > %g x %.3e" % (T, B, e, MARGIN, e_emu)


def test_64_row_tiles_give_the_same_bits(gpu):
    """FR_NJ = 2 (the large-batch tile height) on a small input: the mode has one form per layer and an element's summation order does
    not depend on the tile height, so z is the 32-row result bit for bit -- and within the golden's bar."""
    d, fcfg, wf, emu = golden_case("front_v2_B2_T50")
    fr = hip_front(fcfg, wf, gpu)
    args, fh, nz = golden_args(d, gpu)
    fr.set_option("FR_NJ", 1)
    z1 = fr(*args, fh, noise=nz).cpu()
    fr.set_option("FR_NJ", 2)
    z2 = fr(*args, fh, noise=nz).cpu()
    e = rms(z2, d["z"])
    print("\n[FR_NJ=2] z RMS against the golden %.3e (emulator %.3e); max |NJ=2 - NJ=1| = %.3e" % (e, emu["z"], float((z1 - z2).abs().max())))
    assert e <= MARGIN * emu["z"]
    assert torch.equal(z1, z2)


def test_padding_rows_do_not_leak(gpu):
    d, fcfg, wf, _ = golden_case("front_v2_B2_T50")
    fr = hip_front(fcfg, wf, gpu)
    args, fh, nz = golden_args(d, gpu)
    z0 = fr(*args, fh, noise=nz).cpu()
    L1 = int(d["lengths"][1])
    assert L1 < d["phone"].shape[1]
    phone = args[0].clone()
    phone[1, L1:] = 37.0  # garbage in the padded frames of utterance 1
    z1 = fr(phone, *args[1:], fh, noise=nz).cpu()
    assert torch.equal(z0[0], z1[0])
    assert torch.equal(z0[1, :, :L1], z1[1, :, :L1])
    assert (z1[1, :, L1:] == 0).all()


def test_batch_item_equals_the_single_clip(gpu):
    """B = 2, T = 65 (three time tiles, the last one a single row), ragged, tile height pinned: one launch form per layer, so an item of
    the batch is the same clip run alone bit for bit (the issue's bound is 1e-6)."""
    B, T = 2, 65
    fcfg, wf = FrontConfig(), synth.make_front_weights(FrontConfig(), 77)
    phone, pitch = synth.make_phone(B, T, 768, 9), synth.make_pitch(synth.make_f0(B, T))
    lengths, sid = torch.tensor([T, 50]), torch.tensor([2, 5])
    g = wf["emb_g.weight"][sid].unsqueeze(-1)
    nz = torch.randn(B, 192, T, generator=torch.Generator().manual_seed(8))
    fr = hip_front(fcfg, wf, gpu)
    fr.set_option("FR_NJ", 1)
    z = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), 0, noise=nz.to(gpu)).cpu()
    for b in range(B):
        one = fr(phone[b:b + 1].to(gpu), pitch[b:b + 1].to(gpu), lengths[b:b + 1].to(gpu), g[b:b + 1].to(gpu), 0, noise=nz[b:b + 1].to(gpu)).cpu()
        e = rms(one[0], z[b])
        print("\n[batch item %d against the single clip] RMS %.3e" % (b, e))
        assert e <= 1e-6
        assert torch.equal(one[0], z[b])
    assert float(z[1, :, 50:].abs().max()) == 0.0


def test_no_stale_low_plane_between_handles(gpu):
    """fp16x2 forward, an fp16 handle's forward on other data, the fp16x2 forward again: the first result bit for bit (state is per
    handle, no workspace is shared)."""
    d, fcfg, wf, _ = golden_case("front_v2_B2_T50")
    fr2 = hip_front(fcfg, wf, gpu)
    fr1 = hip_front(fcfg, wf, gpu, operand="fp16")
    args, fh, nz = golden_args(d, gpu)
    z0 = fr2(*args, fh, noise=nz).clone()
    other = (args[0] * 3.0 + 1.0, args[1], None, args[3])
    y = fr1(*other, fh, noise=nz * 2.0)
    assert torch.isfinite(y).all()
    z1 = fr2(*args, fh, noise=nz)
    assert torch.equal(z0, z1)


def test_small_weights_keep_the_precision(gpu):
    """emb_phone.weight x 2^-6 and the phone features x 2^6: the same function in exact arithmetic, with weights whose unscaled low
    parts would all be fp16 subnormals.  z against the golden stays within the golden test's bar."""
    d, fcfg, wf, emu = golden_case("front_v2_B2_T50")
    w = dict(wf)
    w["enc_p.emb_phone.weight"] = wf["enc_p.emb_phone.weight"] * 2.0 ** -6
    assert float(w["enc_p.emb_phone.weight"].abs().max()) * 2.0 ** -11 < 6.1e-5  # every unscaled low part below fp16's smallest normal
    fr = hip_front(fcfg, w, gpu)
    args, fh, nz = golden_args(d, gpu)
    z = fr(args[0] * 2.0 ** 6, *args[1:], fh, noise=nz).cpu()
    e = rms(z, d["z"])
    print("\n[emb_phone.weight x 2^-6, phone x 2^6] z RMS against the golden %.3e (emulator, unscaled: %.3e)" % (e, emu["z"]))
    assert e <= MARGIN * emu["z"]


def test_error_surface(gpu):
    import rvc_amd
    from rvc_amd import _lib

    fcfg = FrontConfig()
    wf = synth.make_front_weights(fcfg, 5)
    fr = hip_front(fcfg, wf, gpu, max_B=2, max_T=96)
    for key, value in (("FR_WN_SPLIT", 2), ("FR_WN_SPLIT", 0), ("FR_FFN_SPLIT", 1), ("FR_NO_FFN_FUSION", 0), ("FR_STAMPS", 1)):
        with pytest.raises(rvc_amd.RvcmiError) as ei:  # a form the mode does not have
            fr.set_option(key, value)
        assert ei.value.code == _lib.ERR_INVALID and "fp16x2" in str(ei.value), str(ei.value)
    for key, value in (("FR_WN_SPLIT", 1), ("FR_FFN_SPLIT", 0), ("FR_NO_FFN_FUSION", 1), ("FR_NJ", 2), ("FR_NJ", None), ("FR_WN_SPLIT", None)):
        fr.set_option(key, value)  # the forms it has, and the defaults
    with pytest.raises(rvc_amd.RvcmiError):
        fr.set_option("FR_NO_SUCH_KEY", 1)
    with pytest.raises(ValueError, match="front-only"):
        rvc_amd.NSFGeneratorHIP(vars(nsf_oracle.CONFIGS["v2_48k"]), {}, device=gpu, operand="fp16x2")
    with pytest.raises(ValueError):
        rvc_amd.FrontHIP(vars(fcfg), wf, device=gpu, operand="fp32")
    fr16 = hip_front(fcfg, wf, gpu, operand="fp16", max_B=2, max_T=96)
    assert fr.workspace_bytes >= fr16.workspace_bytes > 0, (fr.workspace_bytes, fr16.workspace_bytes)
    fr.profile(True)  # profiling names every launch of the mode
    T = 40
    fr(synth.make_phone(1, T, 768, 5).to(gpu), synth.make_pitch(synth.make_f0(1, T)).to(gpu), None, wf["emb_g.weight"][:1].to(gpu), 0)
    names = {s["name"] for s in fr.profile_read()}
    assert {"enc_emb", "enc_qkv", "enc_attn", "enc_o_ln", "enc_ffn1", "enc_ffn2_ln", "enc_proj_zp", "flow_wn_gate", "flow_wn_rs", "flow_post"} <= names, names


class _Net:
    def __init__(self, wf, dec):
        self.emb_g = lambda sid: wf["emb_g.weight"].to(sid.device)[sid]
        self.dec = dec


@pytest.mark.parametrize("name", ["infer_full_v2_48k_T40", "infer_full_v2_48k_rt"])
def test_whole_infer_with_the_fp16x2_front(name, gpu):
    """Whole ``infer`` against the reference's waveform.  fp32 generator: the fp16x2 front's error is at most 1/10 of the fp16 front's.
    Default fp16 generator: at most 1e-3 and not above the fp16 front's."""
    import rvc_amd

    d = load_golden(name)
    fcfg = FrontConfig()
    wf = synth.make_front_weights(fcfg, int(d["seed"]))
    assert synth.weights_sha256(wf) == str(d["front_sha256"])
    cfg = nsf_oracle.CONFIGS["v2_48k"]
    wd = synth.make_dec_weights(cfg, int(d["seed"]))
    assert synth.weights_sha256(wd) == str(d["dec_sha256"])
    T = d["phone"].shape[1]
    opt = lambda k: None if int(d[k]) < 0 else int(d[k])
    fronts = {op: hip_front(fcfg, wf, gpu, operand=op, max_B=1, max_T=128) for op in ("fp16", "fp16x2")}
    err = {}
    for gop in ("fp32", "fp16"):
        dec = rvc_amd.NSFGeneratorHIP(vars(cfg), wd, device=gpu, operand=gop, max_B=1, max_T=128)
        for fop, fr in fronts.items():
            out = rvc_amd.infer_hip(_Net(wf, dec), fr, dev(d, "phone", gpu), torch.tensor([T], device=gpu), dev(d, "sid", gpu), dev(d, "pitch", gpu),
                                    dev(d, "pitchf", gpu), opt("skip_head"), opt("return_length"), opt("return_length2"),
                                    noise_zp=dev(d, "noise_zp", gpu), noise_dec=dev(d, "noise_dec", gpu)).cpu()
            assert out.shape == d["out"].shape
            err[gop, fop] = rms(out, d["out"])
    print("\n[%s] waveform RMS against the reference: fp32 generator: fp16 front %.3e, fp16x2 front %.3e (ratio %.1f); fp16 generator: "
          "fp16 front %.3e, fp16x2 front %.3e" % (name, err["fp32", "fp16"], err["fp32", "fp16x2"], err["fp32", "fp16"] / err["fp32", "fp16x2"],
                                                 err["fp16", "fp16"], err["fp16", "fp16x2"]))
    assert err["fp32", "fp16x2"] * 10 <= err["fp32", "fp16"]
    assert err["fp16", "fp16x2"] <= 1e-3 and err["fp16", "fp16x2"] <= err["fp16", "fp16"]


def test_drop_in_installs_the_fp16x2_front_next_to_the_fp32_generator(rvc_tree, gpu, monkeypatch):  # noqa: F811
    import rvc.synthesizer as ref_syn

    import rvc_amd

    monkeypatch.delenv("RVCMI_FRONT_OPERAND", raising=False)
    d = load_golden("infer_full_v2_48k_T40")
    cpt = make_cpt(int(d["seed"]))
    net_g, _ = ref_syn.get_synthesizer(dict(cpt), gpu)
    rvc_amd.accelerate_synthesizer(net_g, operand="fp32", front_operand=None)  # today's behaviour: the fp32 generator alone
    assert isinstance(net_g.dec, rvc_amd.NSFGeneratorHIP) and net_g.dec.operand == "fp32" and not hasattr(net_g, "_rvcmi_front")
    net_g, _ = ref_syn.get_synthesizer(dict(cpt), gpu)
    rvc_amd.accelerate_synthesizer(net_g, operand="fp32", front_operand="fp16x2")
    assert net_g.dec.operand == "fp32" and isinstance(net_g._rvcmi_front, rvc_amd.FrontHIP) and net_g._rvcmi_front.operand == "fp16x2"
    T = d["phone"].shape[1]
    out = net_g.infer(dev(d, "phone", gpu), torch.tensor([T], device=gpu), dev(d, "sid", gpu), dev(d, "pitch", gpu), dev(d, "pitchf", gpu),
                      noise_zp=dev(d, "noise_zp", gpu), noise_dec=dev(d, "noise_dec", gpu)).cpu()
    e = rms(out, d["out"])
    print("\n[drop-in, fp32 generator + fp16x2 front] waveform RMS against the reference %.3e" % e)
    assert out.shape == d["out"].shape and e <= 1e-3  # the drop-in tests' bar; the fidelity itself is test_whole_infer_with_the_fp16x2_front's
    monkeypatch.setenv("RVCMI_FRONT_OPERAND", "fp16x2")  # the environment switch, through the loader
    net_g, _ = rvc_amd.get_synthesizer(dict(cpt), gpu, operand="fp32")
    assert net_g._rvcmi_front.operand == "fp16x2"
