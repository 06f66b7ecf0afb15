"""What the front's ``"fp16x2"`` operand mode buys in parity, measured on the GPU against the CPU oracle:

* z at T = 1198 (one 10 s clip): RMS against the fp32 oracle and against its fp64 run, fp16 and fp16x2 fronts;
* the 30-clip whole-``infer`` sweep of tests/test_gpu_front.py (same seeds, gains and voiced fractions, fp16 generator) with the fp16 front
  and with the fp16x2 front: worst and median waveform RMS, next to the figures recorded for the fp16 front (9.4e-4 / 5.3e-4).

    python tools/front_split_parity.py --out profiles/front_split_parity.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "front_split_parity.json"))
    ap.add_argument("--seeds", type=int, nargs="*", default=[1234, 7, 99, 2024, 31337])
    ap.add_argument("--T", type=int, default=1198)
    a = ap.parse_args()
    import front_split_cases as fs
    import rvc_amd
    from oracle import front_oracle, nsf_oracle, synth
    from oracle.front_oracle import FrontConfig
    from test_gpu_front import _f0_with_voiced_fraction, _scale_z_path

    assert torch.cuda.is_available(), "this tool measures on the GPU"
    gpu = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    T = a.T
    fcfg, cfg = FrontConfig(), nsf_oracle.CONFIGS["v2_48k"]
    rms = fs.rms
    res = {"device": torch.cuda.get_device_name(0), "T": T, "recorded_fp16_front_sweep": {"worst": 9.4e-4, "median": 5.3e-4}}

    # ---- z at the full clip size ----
    wf = synth.make_front_weights(fcfg, 1234)
    phone = synth.make_phone(1, T, 768, 1234)
    pitch = synth.make_pitch(synth.make_f0(1, T))
    lengths, sid = torch.tensor([T]), torch.tensor([0])
    nz = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(8))
    z32 = fs.run_front("fp32", fcfg, wf, phone, pitch, lengths, sid, nz)
    z64 = fs.run_front("fp32", fcfg, wf, phone, pitch, lengths, sid, nz, dtype=torch.float64)
    g = wf["emb_g.weight"][sid].unsqueeze(-1)
    zrow = {"z_rms": float(z32.pow(2).mean().sqrt()), "fp32_oracle_vs_fp64": rms(z32, z64)}
    for op in ("fp16", "fp16x2"):
        fr = rvc_amd.FrontHIP(vars(fcfg), wf, device=gpu, operand=op, max_B=1, max_T=T)
        z = fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), 0, noise=nz.to(gpu)).cpu()
        zrow[op] = {"vs_fp32_oracle": rms(z, z32), "vs_fp64_oracle": rms(z, z64)}
        del fr
    res["z_T%d" % T] = zrow
    print(json.dumps(zrow), flush=True)

    # ---- the 30-clip sweep ----
    rows = []
    for seed in a.seeds:
        wf, wd0 = synth.make_front_weights(fcfg, seed), synth.make_dec_weights(cfg, seed)
        fronts = {op: rvc_amd.FrontHIP(vars(fcfg), wf, device=gpu, operand=op, max_B=1, max_T=T) for op in ("fp16", "fp16x2")}
        phone = synth.make_phone(1, T, 768, seed)
        lengths, sid = torch.tensor([T]), torch.tensor([seed % 100])
        nz = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(seed + 8))
        noise = nsf_oracle.reference_noise(1, T, cfg.upp, 114514 + seed)
        for frac in (0.2, 0.8):
            pitchf = _f0_with_voiced_fraction(T, frac)
            pitch = synth.make_pitch(pitchf)
            with torch.no_grad():
                zr, m1, g = front_oracle.infer_front(fcfg, wf, phone, pitch, lengths, sid, nz)
            zs = {op: fr(phone.to(gpu), pitch.to(gpu), lengths.to(gpu), g.to(gpu), 0, noise=nz.to(gpu)) for op, fr in fronts.items()}
            for gain in (0.5, 1.0, 2.0):
                wd = _scale_z_path(wd0, gain)
                with torch.no_grad():
                    ref = nsf_oracle.generator_forward(cfg, wd, zr * m1, pitchf, g, noise)
                dec = rvc_amd.NSFGeneratorHIP(vars(cfg), wd, device=gpu, operand="fp16", max_B=1, max_T=T)
                row = {"seed": seed, "gain": gain, "voiced": frac}
                for op in ("fp16", "fp16x2"):
                    out = dec(zs[op], pitchf.to(gpu), g.to(gpu), noise=noise.to(gpu)).cpu()
                    assert torch.isfinite(out).all()
                    row[op] = rms(out, ref)
                del dec
                rows.append(row)
                print(json.dumps(row), flush=True)
    sweep = {"clips": len(rows), "generator": "fp16", "rows": rows}
    for op in ("fp16", "fp16x2"):
        v = sorted(r[op] for r in rows)
        sweep[op + "_front"] = {"worst": v[-1], "median": statistics.median(v), "best": v[0]}
    res["sweep"] = sweep
    print(json.dumps({k: sweep[k] for k in ("fp16_front", "fp16x2_front")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
