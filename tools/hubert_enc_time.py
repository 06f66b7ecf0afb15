"""Times HuBERT's transformer layers: torch's ``.half()`` layers (the path without the switch) against the same layers swapped for
``HubertLayerHIP`` (csrc/hubert_enc.hip) with the same weights, in one process, the two alternating; then the whole
``transformers.HubertModel`` (random weights: cost only) with the layer swap off / on, each with and without the extractor swap
(``RVCMI_HUBERT_FE``'s ``accelerate_hubert``).

    python tools/hubert_enc_time.py --out profiles/hubert_enc_time.json

Per shape: median and range over ``--repeats`` timed calls after ``--warmup`` untimed ones, device-synchronised host clock.  The verdict is
"hip faster" / "torch faster" only when the two ranges are disjoint, else "tie".  A whole conversion (``bench.py --e2e``) is not timed here.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from hubert_fe_time import alternate, verdict  # noqa: E402

# (label, B, frames): one second, the realtime window, a 12 s clip, a 71 s segment, a group of eight 12 s clips
SHAPES = (("1s", 1, 49), ("realtime_window", 1, 137), ("12s", 1, 599), ("71s", 1, 3549), ("8x12s", 8, 599))


def samples(frames):
    return 400 + 320 * (frames - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_enc_time.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import rvc_amd
    from transformers import HubertConfig, HubertModel

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = HubertModel(HubertConfig()).eval().half().to(dev)
    layers = model.encoder.layers
    originals = list(layers)
    assert rvc_amd.accelerate_hubert_layers(model) == len(originals), "the layers were not recognised"
    swapped = list(layers)
    enc = swapped[0].encoder
    rvc_amd.restore_hubert_layers(model)

    def stack(mods, x):
        for m in mods:
            x = m(x)[0]
        return x

    def set_layers(mods):
        for i, m in enumerate(mods):
            layers[i] = m

    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "layers": len(originals), "stack": [], "model": [],
           "method": "same process, alternating torch / HIP, device-synchronised host clock; stack = the 12 layer modules called in a loop on a "
                     "[B, frames, 768] fp16 tensor: torch = HubertEncoderLayer.half(), hip = HubertLayerHIP (one forward of one layer each, output "
                     "allocation included), hip_one_call = HubertEncoderHIP.forward over all 12 layers; model = HubertModel.half() forward, random weights"}
    with torch.no_grad():
        for label, B, T in SHAPES:
            x = torch.randn(B, T, 768, device=dev).half()
            t, h = alternate(lambda: stack(originals, x), lambda: stack(swapped, x), a.warmup, a.repeats)
            _, one = alternate(lambda: None, lambda: enc(x), a.warmup, a.repeats)
            flops = 12.0 * B * T * 2.0 * (4 * 768 * 768 + 2 * 768 * 3072 + 2 * T * 768)
            row = {"label": label, "B": B, "frames": T, "torch_half": t, "hip": h, "hip_one_call": one, "verdict": verdict(t, h),
                   "speedup_median": t["median_ms"] / h["median_ms"], "flops": flops, "hip_tflops": flops / h["median_ms"] / 1e9,
                   "workspace_bytes": enc.workspace_bytes(B, T)}
            res["stack"].append(row)
            print(json.dumps(row), flush=True)
        for fe_on in (False, True):
            if fe_on:
                assert rvc_amd.accelerate_hubert(model) == 1
            for label, B, T in SHAPES:
                x = (0.1 * torch.randn(B, samples(T), device=dev)).half()

                def run_off():
                    set_layers(originals)
                    return model(x).last_hidden_state

                def run_on():
                    set_layers(swapped)
                    return model(x).last_hidden_state

                t, h = alternate(run_off, run_on, a.warmup, a.repeats)
                set_layers(originals)
                row = {"label": label, "B": B, "frames": T, "hubert_fe": fe_on, "switch_off": t, "switch_on": h, "verdict": verdict(t, h),
                       "speedup_median": t["median_ms"] / h["median_ms"]}
                res["model"].append(row)
                print(json.dumps(row), flush=True)
        rvc_amd.restore_hubert(model)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
