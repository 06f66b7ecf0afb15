"""Writes the fixtures of the RMVPE U-Net tests from the REAL reference modules, on the CPU in fp32:

    python tools/make_golden_unet.py /path/to/Retrieval-based-Voice-Conversion-WebUI

  tests/golden/rmvpe_unet_keys.json     the ``unet.*`` / ``cnn.*`` state-dict keys of ``E2E(4, 1, (2, 2))`` with their shapes, in order
  tests/golden/rmvpe_unet_T32.npz       seeded mel [1, 128, 32] and the real modules' output [1, 32, 384] for ``seeded_weights(keys, SEED)``
  tests/golden/rmvpe_unet_small_T24.npz the same for a reduced network ``E2E(2, 1, (2, 2), en_de_layers=3, inter_layers=2)``

The reference's ``rvc/f0/deepunet.py`` and ``e2e.py`` need only torch, but the package's ``__init__`` imports librosa; the two files are
therefore loaded under a stand-in package name.  Nothing of the reference is copied: it is read and run here, only its outputs are kept.
The weights are loaded with ``load_state_dict(strict=True)``, which also proves the key list.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import unet_cases as uc  # noqa: E402

SEED, MEL_SEED = 20240, 7


def load_reference(ref_root):
    pkg = types.ModuleType("_ref_f0")
    pkg.__path__ = [os.path.join(ref_root, "rvc", "f0")]
    sys.modules["_ref_f0"] = pkg
    mods = {}
    for name in ("deepunet", "e2e"):
        spec = importlib.util.spec_from_file_location("_ref_f0." + name, os.path.join(ref_root, "rvc", "f0", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules["_ref_f0." + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["e2e"].E2E


def case(E2E, args, kwargs, T, seed, mel_seed):
    torch.manual_seed(0)
    model = E2E(*args, **kwargs).eval()
    full = model.state_dict()
    keys = [(k, tuple(v.shape)) for k, v in full.items() if k.startswith("unet.") or k.startswith("cnn.")]
    sd = uc.seeded_weights(keys, seed)
    full.update(sd)
    model.load_state_dict(full, strict=True)
    mel = uc.seeded_mel(1, T, mel_seed)
    with torch.no_grad():
        x = mel.transpose(-1, -2).unsqueeze(1)
        out = model.cnn(model.unet(x)).transpose(1, 2).flatten(-2)
    return keys, mel, out


def main():
    E2E = load_reference(sys.argv[1])
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    keys, mel, out = case(E2E, (4, 1, (2, 2)), {}, 32, SEED, MEL_SEED)
    assert keys == uc.key_list(**uc.FULL), "tests/unet_cases.key_list does not describe the reference's network"
    g = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(g, "rmvpe_unet_keys.json"), "w") as f:
        json.dump([[k, list(s)] for k, s in keys], f, indent=0)
        f.write("\n")
    np.savez_compressed(os.path.join(g, "rmvpe_unet_T32.npz"), mel=mel.numpy(), out=out.numpy(), seed=SEED, mel_seed=MEL_SEED)
    small = dict(levels=3, blocks=2, inters=2, base=16)
    keys2, mel2, out2 = case(E2E, (2, 1, (2, 2)), dict(en_de_layers=3, inter_layers=2), 24, SEED + 1, MEL_SEED + 1)
    assert keys2 == uc.key_list(**small)
    np.savez_compressed(os.path.join(g, "rmvpe_unet_small_T24.npz"), mel=mel2.numpy(), out=out2.numpy(), seed=SEED + 1, mel_seed=MEL_SEED + 1,
                        **{k: np.int64(v) for k, v in small.items()})
    print("%d keys; T32 out rms %.4f, small out rms %.4f" % (len(keys), float(out.pow(2).mean().sqrt()), float(out2.pow(2).mean().sqrt())))


if __name__ == "__main__":
    main()
