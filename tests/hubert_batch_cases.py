"""Shared pieces of the batched-HuBERT tests (tests/test_cpu_hubert_batch.py, tests/test_gpu_hubert_batch.py) and of
tools/hubert_batch_parity.py / tools/hubert_batch_time.py: fairseq's padding-mask rule restated, a fairseq-shaped model around the modules of
transformers' ``HubertModel``, the groups of lengths, and the whole-model error measurement.

The wrapper is written here, not taken from transformers' encoder: ``forward_padding_mask`` (the sample mask -> frame mask rule), the
zeroing of padded frames in front of the positional convolution and the masking of padded attention KEYS are the three things a padded batch
rests on, and the tests need a model that does exactly these and nothing more.  It runs in any float dtype on any device, so the same class
in fp64 on the CPU is the reference the fp32 GPU legs are measured against.
"""
import copy
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import hubert_cases as hc  # noqa: E402

# (5040, 400, 1040): one / three frames next to fifteen.  (21000, ...): 3, 1, 2 and 2 statistics chunks of 2048 layer-0 frames -- chunks wholly
# behind an item's end.  (41360, ...): 129, 128, 127 and 1 final rows -- a partial last-layer tile, one wholly behind an item's end.
GROUPS = ((5040, 400, 1040), (21000, 400, 10250, 10649), (41360, 41040, 40720, 400))
MODEL_GROUPS = ((5040, 400, 1040), (41360, 41040, 400))
GAINS = hc.ITEM_GAINS + (0.5,)
SMALL = dict(num_hidden_layers=2, hidden_size=64, num_attention_heads=4, intermediate_size=128, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4)


def fairseq_frame_mask(sample_mask, L):
    """fairseq's ``HubertModel.forward_padding_mask``: drop the ``N % L`` tail, ``view(B, L, -1).all(-1)``."""
    extra = sample_mask.size(1) % L
    if extra > 0:
        sample_mask = sample_mask[:, :-extra]
    return sample_mask.view(sample_mask.size(0), L, -1).all(-1)


def naive_sample_mask(lens, N_max):
    """True from sample ``lens[i]`` on: what a caller writes without thinking about the rule above."""
    return torch.arange(N_max).unsqueeze(0) >= torch.tensor(list(lens)).unsqueeze(1)


def waves(lens, seed=0):
    """-> one float32 numpy waveform per length: white noise of amplitude 0.5, item i scaled by GAINS[i]"""
    rng = np.random.default_rng(2000 + seed)
    return [(0.5 * GAINS[i % len(GAINS)] * rng.uniform(-1.0, 1.0, n)).astype(np.float32) for i, n in enumerate(lens)]


class MaskBlind(torch.nn.Module):
    """The modules of a transformers ``HubertModel`` (post-norm, ``feat_proj_layer_norm``) behind fairseq's interface:
    ``extract_features(source, padding_mask, output_layer) -> (x [B, L, d], frame_mask)``, ``forward_padding_mask``, ``final_proj``.  This base class has NO ``forward_padding_mask`` and ignores ``padding_mask`` -- the shape of a model that must stay on the per-item loop;
    ``FairseqShaped`` below adds the method."""

    def __init__(self, hf):
        super().__init__()
        assert not hf.config.do_stable_layer_norm and hf.config.feat_proj_layer_norm
        self.feature_extractor = hf.feature_extractor
        self.layer_norm = hf.feature_projection.layer_norm
        self.post_extract_proj = hf.feature_projection.projection
        self.pos_conv = hf.encoder.pos_conv_embed
        self.encoder_norm = hf.encoder.layer_norm
        self.layers = hf.encoder.layers
        self.heads = hf.config.num_attention_heads
        self.final_proj = torch.nn.Linear(hf.config.hidden_size, 256)

    def _attention(self, att, x, key_mask):
        B, L, d = x.shape
        hd = d // self.heads
        q = att.q_proj(x).view(B, L, self.heads, hd).transpose(1, 2) * hd ** -0.5
        k = att.k_proj(x).view(B, L, self.heads, hd).transpose(1, 2)
        v = att.v_proj(x).view(B, L, self.heads, hd).transpose(1, 2)
        s = q @ k.transpose(-1, -2)
        if key_mask is not None:
            s = s.masked_fill(key_mask[:, None, None, :], -math.inf)
        return att.out_proj((torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, L, d))

    def encode(self, rows, frame_mask=None, output_layer=None):
        """``rows`` [B, L, 512]: the extractor's output, channels last -> [B, L, d]"""
        x = self.post_extract_proj(self.layer_norm(rows))
        if frame_mask is not None:
            x = x.masked_fill(frame_mask.unsqueeze(-1), 0.0)
        x = self.encoder_norm(x + self.pos_conv(x))
        for layer in list(self.layers)[:output_layer]:
            x = layer.layer_norm(x + self._attention(layer.attention, x, frame_mask))
            ff = layer.feed_forward
            x = layer.final_layer_norm(x + ff.output_dense(torch.nn.functional.gelu(ff.intermediate_dense(x))))
        return x

    def extract_features(self, source, padding_mask=None, output_layer=None):
        dtype = self.layer_norm.weight.dtype
        rows = self.feature_extractor(source.to(dtype)).transpose(1, 2)
        fm = None
        if padding_mask is not None and bool(padding_mask.any()) and hasattr(self, "forward_padding_mask"):
            fm = self.forward_padding_mask(rows, padding_mask)
        return self.encode(rows, fm, output_layer), fm


class FairseqShaped(MaskBlind):
    def forward_padding_mask(self, features, padding_mask):
        return fairseq_frame_mask(padding_mask, features.size(1))


def make_model(device, seed=3, with_padding_mask=True, **cfg):
    from transformers import HubertConfig, HubertModel

    torch.manual_seed(seed)
    return (FairseqShaped if with_padding_mask else MaskBlind)(HubertModel(HubertConfig(**{**SMALL, **cfg})).eval()).eval().to(device)


def reference_of(model):
    """The encoder of ``model`` in fp64 on the CPU (made BEFORE the extractor is swapped: a HIP handle cannot be copied); it has no extractor."""
    fe, model.feature_extractor = model.feature_extractor, None
    try:
        ref = copy.deepcopy(model)
    finally:
        model.feature_extractor = fe
    return ref.double().cpu()


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a)))


def whole_model_errors(gpu, lens, output_layer=12, naive=False, seed=3):
    """Per item of the group ``lens``: ``e_batch`` = RMS(batched - ref64), ``e_single`` = RMS(lone call - ref64), ``ref_rms``.  ref64: the fp64 CPU encoder fed with the item's extractor rows from
    the dense HIP entry on the item alone (the batched leg's rows are those bit for bit: test_gpu_hubert_batch.py's first test).  ``naive``: the batched leg with the plain
    sample mask instead of ``hubert.sample_mask``.  Inputs under ``hubert.MIN_SAMPLES`` stay on the kernels here (the threshold is set aside for the measurement)."""
    import rvc_amd
    from rvc_amd import hubert

    model = make_model(gpu, seed)
    ref = reference_of(model)
    assert rvc_amd.accelerate_hubert(model) == 1 and hubert.batch_capable(model)
    fe = model.feature_extractor
    ws = [torch.from_numpy(w).to(gpu) for w in waves(lens, seed)]
    keep, hubert.MIN_SAMPLES = hubert.MIN_SAMPLES, 0
    try:
        with torch.no_grad():
            if naive:
                x = torch.zeros(len(lens), max(lens), device=gpu)
                for i, w in enumerate(ws):
                    x[i, :lens[i]] = w
                with fe.ragged(lens):
                    y = model.extract_features(source=x, padding_mask=naive_sample_mask(lens, max(lens)).to(gpu), output_layer=output_layer)[0]
                batched = [y[i:i + 1, :hubert.frames(n)] for i, n in enumerate(lens)]
            else:
                batched = hubert.extract_features_batch(model, ws, output_layer)
            out = []
            for i, w in enumerate(ws):
                x = w.view(1, -1)
                rows = fe(x).transpose(1, 2)
                want = ref.encode(rows.double().cpu(), None, output_layer).numpy()
                single = model.extract_features(source=x, padding_mask=torch.zeros_like(x, dtype=torch.bool), output_layer=output_layer)[0]
                assert tuple(batched[i].shape) == tuple(single.shape) == want.shape == (1, hubert.frames(lens[i]), want.shape[2])
                out.append({"len": int(lens[i]), "frames": int(want.shape[1]), "e_batch": rms(batched[i].double().cpu().numpy() - want),
                            "e_single": rms(single.double().cpu().numpy() - want), "ref_rms": rms(want)})
    finally:
        hubert.MIN_SAMPLES = keep
        rvc_amd.restore_hubert(model)
    return out


def within_bar(e):
    """Only the GEMMs' M and the (exactly zero) masked terms of the softmax sums differ between the legs: a factor of 2 is summation-order room."""
    return e["e_batch"] <= 2.0 * e["e_single"] + 1e-6 * e["ref_rms"]
