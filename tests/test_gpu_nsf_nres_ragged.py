"""The generator's realtime interpolation with a target PER ITEM (``rvcmi_nsf_forward_nres``; Python: ``n_res`` = a sequence): one call
decodes every item of a batch to its own ``return_length2`` -- the ragged partial decode a bank's per-session formant shift needs.
Item b must be the single-item call with ``n_res[b]`` bit for bit (kernel family pinned as tests/test_gpu_generator.py pins it for its
ragged batches), the samples behind its end zero, and one item must meet the oracle under that file's bars."""
import pytest
import torch

from conftest import rms
from oracle import nsf_oracle, synth
from oracle.nsf_oracle import GenConfig

pytestmark = pytest.mark.gpu

# fp16 families: a longer item, an equal one (not interpolated at all), a shorter one, a single frame, one frame past T
NRES = {"tiles": (64, [72, 64, 57, 1, 65]), "stream": (64, [72, 64, 57, 1, 65]), "fp32": (16, [18, 16, 14, 1])}
BAR = {"fp32": 2e-5, "tiles": 1e-3, "stream": 1e-3}


def pin(gen, **opts):
    """Test options of ONE handle, the recipe of tests/test_gpu_generator.py: RB_STREAM 1 / 0 forces the streaming / the tile ResBlock kernels,
    NO_RB_SPLIT keeps the short-launch split path out, so that a batch and its single-item calls run the same kernel family."""
    for k, v in opts.items():
        gen.set_option(k, v)
    return gen


def _inputs(cfg, B, T, gpu):
    zs, fs, gs, ns = [], [], [], []
    for b in range(B):
        z, f0, g = synth.make_dec_inputs(cfg, 1, T, 500 + b)
        zs.append(z), gs.append(g)
        if cfg.use_f0:
            fs.append(torch.roll(f0, 11 * b, dims=1))
            ns.append(nsf_oracle.reference_noise(1, T, cfg.upp, 900 + b))
    cat = lambda v: torch.cat(v).to(gpu) if v else None  # noqa: E731
    return (zs, fs, gs, ns), (cat(zs), cat(fs), cat(gs), cat(ns))


@pytest.mark.parametrize("family", ["tiles", "stream", "fp32"])
def test_per_item_n_res_equals_the_single_item_calls_bit_for_bit(family, gpu):
    import rvc_amd

    cfg = nsf_oracle.CONFIGS["v2_48k"]
    w = synth.make_dec_weights(cfg, 99)
    T, nres = NRES[family]
    B, Tmax = len(nres), max(nres)
    host, (Z, F, G, N) = _inputs(cfg, B, T, gpu)
    gen = rvc_amd.NSFGeneratorHIP(vars(cfg), w, device=gpu, operand="fp32" if family == "fp32" else "fp16", max_B=B, max_T=Tmax)
    if family != "fp32":
        pin(gen, RB_STREAM=1 if family == "stream" else 0, NO_RB_SPLIT=1)
    out = gen(Z, F, G, nres, noise=N)
    assert out.shape == (B, 1, Tmax * cfg.upp) and bool(torch.isfinite(out).all())
    assert torch.equal(out, gen(Z, F, G, torch.tensor(nres), noise=N))            # a tensor is a sequence too; the cached device copy
    for b, n in enumerate(nres):
        one = gen(Z[b:b + 1], F[b:b + 1], G[b:b + 1], n, noise=N[b:b + 1])
        assert one.shape == (1, 1, n * cfg.upp)
        assert torch.equal(one[0, 0], out[b, 0, :n * cfg.upp]), "item %d (n_res %d of T %d) differs from its single-item call: rms %.3e" % (
            b, n, T, rms(one[0, 0].cpu(), out[b, 0, :n * cfg.upp].cpu()))
        assert not out[b, 0, n * cfg.upp:].any(), "item %d: samples behind its end" % b
    assert torch.equal(gen(Z[1:2], F[1:2], G[1:2], noise=N[1:2])[0, 0], out[1, 0, :T * cfg.upp])   # n_res == T: no interpolation at all
    # the oracle (= the reference's arithmetic) on the longer item, run alone
    zs, fs, gs, ns = host
    with torch.no_grad():
        ref = nsf_oracle.generator_forward(cfg, w, zs[0], fs[0], gs[0], ns[0], n_res=nres[0])
    e = rms(out[0:1, :, :nres[0] * cfg.upp].cpu(), ref)
    print("%s: item 0 (n_res %d) rms %.3e against the oracle, bar %.0e" % (family, nres[0], e, BAR[family]))
    assert e <= BAR[family]
    # what stays refused
    with pytest.raises(ValueError):
        gen(Z, F, G, nres, noise=N, lengths=torch.tensor([T] * B))
    with pytest.raises(ValueError):
        gen(Z, F, G, 10, noise=N, lengths=torch.tensor([T] * B))
    with pytest.raises(ValueError):
        gen(Z, F, G, nres[:-1], noise=N)
    with pytest.raises(ValueError):
        gen(Z, F, G, [0] + nres[1:], noise=N)
    with pytest.raises(ValueError):
        gen(Z, F, G, [Tmax + 1] + nres[1:], noise=N)
    with pytest.raises(ValueError):
        gen.debug_tap("pre", Z, F, G, nres, N)


def test_per_item_n_res_without_f0(gpu):
    """The no-f0 ``GeneratorHIP`` (generators.py:76-79: only x is interpolated)."""
    import rvc_amd

    cfg = GenConfig(**{**vars(nsf_oracle.CONFIGS["v2_48k"]), "use_f0": False})
    w = synth.make_dec_weights(cfg, 99)
    T, nres = 16, [18, 16, 13, 1]
    B = len(nres)
    host, (Z, _, G, _) = _inputs(cfg, B, T, gpu)
    gen = rvc_amd.GeneratorHIP(vars(cfg), w, device=gpu, operand="fp16", max_B=B, max_T=max(nres))
    pin(gen, RB_STREAM=0, NO_RB_SPLIT=1)
    out = gen(Z, G, nres)
    assert out.shape == (B, 1, max(nres) * cfg.upp) and bool(torch.isfinite(out).all())
    for b, n in enumerate(nres):
        one = gen(Z[b:b + 1], G[b:b + 1], n)
        assert torch.equal(one[0, 0], out[b, 0, :n * cfg.upp]), "item %d" % b
        assert not out[b, 0, n * cfg.upp:].any()
    with torch.no_grad():
        ref = nsf_oracle.generator_forward(cfg, w, host[0][0], None, host[2][0], None, n_res=nres[0])
    assert rms(out[0:1, :, :nres[0] * cfg.upp].cpu(), ref) <= 1e-3
    with pytest.raises(ValueError):
        gen(Z, G, nres, lengths=torch.tensor([T] * B))


def test_forward_nres_rejects_bad_arguments_at_the_c_abi(gpu):
    import rvc_amd
    from rvc_amd import _lib

    cfg = nsf_oracle.CONFIGS["v2_48k"]
    B, T, max_T = 2, 8, 10
    gen = rvc_amd.NSFGeneratorHIP(vars(cfg), synth.make_dec_weights(cfg, 99), device=gpu, operand="fp16", max_B=B, max_T=max_T)
    _, (Z, F, G, N) = _inputs(cfg, B, T, gpu)
    G = G.reshape(B, -1).contiguous()
    nres = torch.tensor([9, 7], dtype=torch.int32, device=gpu)
    out = torch.zeros(B, (max_T + 1) * cfg.upp, device=gpu)
    L, p, st, h = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu), gen._handle
    with torch.cuda.device(gpu):
        call = lambda b, t, nmax, nr: L.rvcmi_nsf_forward_nres(h, b, t, nmax, nr, p(Z), p(F), p(G), p(N), p(out), st)  # noqa: E731
        assert call(B, T, 9, p(nres)) == 0
        assert call(0, T, 9, p(nres)) == _lib.ERR_INVALID
        assert call(B, T, 0, p(nres)) == _lib.ERR_INVALID
        assert call(B, T, 9, None) == _lib.ERR_INVALID
        assert call(B, T, max_T + 1, p(nres)) == _lib.ERR_NOMEM
        assert call(B + 1, T, 9, p(nres)) == _lib.ERR_NOMEM
        # the existing entry point keeps refusing lengths together with n_res
        assert L.rvcmi_nsf_forward(h, B, T, p(nres), p(Z), p(F), p(G), p(N), 9, p(out), st) == _lib.ERR_INVALID
    torch.cuda.synchronize(gpu)
    item1 = out.reshape(-1)[9 * cfg.upp: 18 * cfg.upp]   # the one call that ran wrote rows of n_res_max = 9 frames
    assert bool(torch.isfinite(out).all()) and not item1[7 * cfg.upp:].any() and bool(item1[:7 * cfg.upp].any())
