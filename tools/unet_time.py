"""Time and parity of the RMVPE U-Net on csrc/unet.hip against the path it replaces: torch / MIOpen ``.half()`` U-Net + head, same weights.

    python tools/unet_time.py --out profiles/unet_time.json [--parity profiles/unet_parity.json] [--repeats 20]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/unet_time.py --trace 1,1024      (HIP forwards only, for the kernel statistics)

Both legs run in ONE process, alternating A / B, every shape warmed up first, timed with a device-synchronised host clock; median and range
of ``--repeats`` runs per leg.  A shape whose ranges overlap is a tie.  One more leg times the f0 step ``pipeline._rmvpe_on_device`` with the
switch off and on (a stand-in RMVPE object: the mel front end of tools/e2e_proxies.py, the recognised network, the HIP GRU).

    python tools/unet_time.py --rates profiles/unet_kernel_stats.csv --trace 1,1024 --out profiles/unet_kernel_rates.json      (no GPU)

Operation and byte counts per kernel come from the layer shapes (``counts``): FLOPs = 2 * output pixels * Cout * taps * Cin; bytes = weights
once + inputs once + outputs once (the minimum traffic; re-reads of the 3x3 halo come from the caches); a layer that splits its K loop
writes fp32 partials instead, which ``k_unet_reduce`` reads back (the split rule of csrc/unet.hip is restated in ``counts`` and checked
against the launch counts of the kernel statistics by ``--rates``).
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import unet_cases as uc  # noqa: E402

SHAPES = [(1, 32), (1, 64), (1, 1024), (1, 3072), (8, 1024)]
PEAK_FP16_FLOPS, PEAK_HBM_BYTES = 2.5e15, 8.0e12  # MI355X: dense fp16 MFMA, HBM3E


def counts(B, T, levels=5, blocks=4, inters=4, base=16, head=3):
    """Per kernel (as csrc/unet.hip picks them): launches, FLOPs, minimum bytes of one forward."""
    out = {}

    def add(name, flops, nbytes):
        e = out.setdefault(name, dict(launches=0, flops=0.0, bytes=0.0))
        e["launches"] += 1
        e["flops"] += flops
        e["bytes"] += nbytes

    def conv(pix, cin, cout, taps, up=False, res=False, head_out=False):
        cfg = 0 if cout <= 16 else 1 if cout <= 32 else 2
        name = ("k_unet_conv<1,1>", "k_unet_conv<2,1>", "k_unet_conv<2,2>")[cfg]
        opix = 4 * pix if up else pix
        t = 9 / 4.0 if up else taps
        # the K split of csrc/unet.hip (conv()): fewer than 128 blocks -> up to 32 slices of at least 4 K steps
        pix_blk, co_blk = (128, 128, 64)[cfg], (16, 32, 64)[cfg]
        blocks = -(-pix // pix_blk) * -(-cout // co_blk) * (4 if up else 1)
        ksplit = 1
        if not head_out and cout % 16 == 0 and blocks < 128:
            ksplit = max(1, min(-(-256 // blocks), 32, ((4 if up else taps) * -(-cin // 32)) // 4))
        w_in = 2.0 * (9 if up else taps) * cin * cout + 2.0 * pix * cin
        if ksplit == 1:
            add(name, 2.0 * opix * cout * t * cin, w_in + (4.0 if head_out else 2.0) * opix * cout + (2.0 * opix * cout if res else 0))
        else:  # fp32 partials out of the convolution, summed in slice order by the reduction, which also applies the epilogue
            add(name, 2.0 * opix * cout * t * cin, w_in + 4.0 * ksplit * opix * cout)
            add("k_unet_reduce", (ksplit + 2.0) * opix * cout, 4.0 * ksplit * opix * cout + 2.0 * opix * cout + (2.0 * opix * cout if res else 0))

    def unit(pix, cin, cout):
        if cin == 1:
            add("k_unet_first", 2.0 * pix * cout * 9, 4.0 * pix + 2.0 * pix * cout)
            add("k_unet_first", 2.0 * pix * cout, 4.0 * pix + 2.0 * pix * cout)
        else:
            conv(pix, cin, cout, 9)
            if cin != cout:
                conv(pix, cin, cout, 1)
        conv(pix, cout, cout, 9, res=True)

    pix, cin, c = B * T * 128, 1, base
    for _ in range(levels):
        for u in range(blocks):
            unit(pix, c if u else cin, c)
        add("k_unet_pool", pix * c, 2.0 * pix * c * 1.25)
        pix, cin, c = pix // 4, c, 2 * c
    for i in range(inters):
        for u in range(blocks):
            unit(pix, c if (i or u) else cin, c)
    for _ in range(levels):
        conv(pix, c, c // 2, 9, up=True)
        pix, c = pix * 4, c // 2
        for u in range(blocks):
            unit(pix, c if u else 2 * c, c)
    conv(pix, base, head, 9, head_out=True)
    return out


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def leg(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def verdict(a, b):
    if a["max_ms"] < b["min_ms"]:
        return "hip faster"
    if b["max_ms"] < a["min_ms"]:
        return "torch faster"
    return "tie"


class E2ELike(uc.StandIn):
    def __init__(self, keys, sd):
        super().__init__(keys, sd)
        torch.manual_seed(5)
        self.gru = torch.nn.GRU(384, 256, num_layers=1, batch_first=True, bidirectional=True)
        self.out = torch.nn.Linear(512, 360)

    def forward(self, mel):
        return torch.sigmoid(self.out(self.gru(super().forward(mel))[0]))


def rates(a):
    """Per kernel of one forward at the traced shape: launches, time, achieved FLOP/s and bytes/s (counts from the shapes, times from the
    kernel statistics) and the fraction of the bound that is closer."""
    import csv

    B, T = (int(v) for v in a.trace.split(","))
    cn = counts(B, T)
    rows = {}
    for r in csv.DictReader(open(a.rates)):
        for k in cn:
            if k.replace(",", ", ") in r["Name"] or (k.find("<") < 0 and k in r["Name"]):
                rows[k] = r
    out = dict(shape=dict(B=B, T=T), forwards=a.forwards, source=os.path.basename(a.rates), kernels={}, peak_fp16_flops=PEAK_FP16_FLOPS, peak_hbm_bytes=PEAK_HBM_BYTES)
    for k, c in cn.items():
        r = rows[k]
        assert int(r["Calls"]) == a.forwards * c["launches"], (k, r["Calls"], c["launches"])
        sec = float(r["TotalDurationNs"]) * 1e-9 / a.forwards
        ff, fb = c["flops"] / sec / PEAK_FP16_FLOPS, c["bytes"] / sec / PEAK_HBM_BYTES
        out["kernels"][k] = dict(launches=c["launches"], us_per_forward=sec * 1e6, us_per_launch=sec * 1e6 / c["launches"], tflops=c["flops"] / sec / 1e12,
                                 min_traffic_gbs=c["bytes"] / sec / 1e9, frac_of_fp16_peak=ff, frac_of_hbm_peak=fb, nearer_bound="hbm" if fb > ff else "fp16 mfma")
    out["launches_per_forward"] = sum(c["launches"] for c in cn.values())
    out["kernel_us_per_forward"] = sum(v["us_per_forward"] for v in out["kernels"].values())
    json.dump(out, open(a.out, "w"), indent=1)
    for k, v in out["kernels"].items():
        print("%-18s %3d launches %8.1f us  %7.2f TFLOP/s (%.2f %%)  %7.1f GB/s (%.2f %%)" % (k, v["launches"], v["us_per_forward"], v["tflops"], 100 * v["frac_of_fp16_peak"],
                                                                                              v["min_traffic_gbs"], 100 * v["frac_of_hbm_peak"]))
    print("launches per forward", out["launches_per_forward"], "kernel us per forward %.1f" % out["kernel_us_per_forward"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parity")
    ap.add_argument("--trace")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rates", help="a rocprofv3 kernel_stats.csv of a --trace run: per-kernel achieved rates against the bounds -> --out (no GPU needed)")
    ap.add_argument("--forwards", type=int, default=5)
    a = ap.parse_args()
    if a.rates:
        return rates(a)
    import rvc_amd
    import rvc_amd.pipeline as rp

    dev = torch.device("cuda:0")
    keys = uc.golden_keys()
    sd = uc.seeded_weights(keys, 20240)
    hip = rvc_amd.UNetHIP.from_state_dict(sd, dev)
    if a.trace:
        B, T = (int(v) for v in a.trace.split(","))
        x = uc.seeded_mel(B, T, 1).to(dev).half().transpose(-1, -2).unsqueeze(1)
        for _ in range(5):
            hip(x)
        torch.cuda.synchronize(dev)
        return
    sd16 = uc.to(sd, dev, torch.float16)
    res = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, warmup=a.warmup, shapes=[],
               method="same process, alternating torch / HIP, device-synchronised host clock; torch = F.conv2d / batch_norm / relu / avg_pool2d / "
                      "conv_transpose2d / cat on .half() weights (MIOpen), HIP = UNetHIP.forward incl. its workspace allocation and dtype casts")
    with torch.no_grad():
        for B, T in SHAPES:
            mel = uc.seeded_mel(B, T, T).to(dev).half()
            x = mel.transpose(-1, -2).unsqueeze(1)
            fa = lambda: uc.head_forward(sd16, uc.unet_forward(sd16, x))  # noqa: E731
            fb = lambda: hip(x)  # noqa: E731
            for _ in range(a.warmup):
                timed(fa, dev), timed(fb, dev)
            ta, tb = [], []
            for _ in range(a.repeats):
                ta.append(timed(fa, dev))
                tb.append(timed(fb, dev))
            la, lb = leg(ta), leg(tb)
            cn = counts(B, T)
            flops, nbytes = sum(v["flops"] for v in cn.values()), sum(v["bytes"] for v in cn.values())
            row = dict(B=B, T=T, launches=sum(v["launches"] for v in cn.values()), torch_half=la, hip=lb, verdict=verdict(lb, la), speedup_median=la["median_ms"] / lb["median_ms"], flops=flops, min_bytes=nbytes,
                       hip_tflops=flops / lb["median_ms"] / 1e9, hip_min_traffic_gbs=nbytes / lb["median_ms"] / 1e6,
                       frac_of_fp16_peak=flops / (lb["median_ms"] * 1e-3) / PEAK_FP16_FLOPS, frac_of_hbm_peak=nbytes / (lb["median_ms"] * 1e-3) / PEAK_HBM_BYTES,
                       workspace_bytes=hip.workspace_bytes(B, T), kernels=cn)
            print(json.dumps({k: v for k, v in row.items() if k != "kernels"}), flush=True)
            res["shapes"].append(row)
        # the f0 step of the pipeline, switch off / on
        from e2e_proxies import RmvpeProxy

        f0 = {}
        for secs in (2, 10):
            audio = (0.3 * torch.sin(2 * torch.pi * 220.0 * torch.arange(16000 * secs) / 16000.0)).to(dev)
            p_len = audio.shape[0] // 160
            legs = {}
            mes = {}
            for sw in ("0", "1"):
                os.environ["RVCMI_RMVPE_UNET"] = sw
                r = RmvpeProxy(dev, half=True)
                r.model = E2ELike(keys, sd).eval().to(dev).half()
                mes[sw] = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=r, is_half=True, device=dev))
                for _ in range(a.warmup):
                    rp._rmvpe_on_device(mes[sw], audio, p_len, 0)
                assert getattr(r, "_rvcmi_unet", 0) == int(sw)
                legs[sw] = []
            for _ in range(a.repeats):
                for sw in ("0", "1"):
                    os.environ["RVCMI_RMVPE_UNET"] = sw  # (the helper reads the switch on every call)
                    legs[sw].append(timed(lambda: rp._rmvpe_on_device(mes[sw], audio, p_len, 0), dev))
            assert getattr(mes["0"].f0_gen.rmvpe, "_rvcmi_unet", 0) == 0 and mes["1"].f0_gen.rmvpe._rvcmi_unet == 1
            off, on = leg(legs["0"]), leg(legs["1"])
            f0["%ds" % secs] = dict(seconds=secs, switch_off=off, switch_on=on, verdict=verdict(on, off))
            print(json.dumps(f0["%ds" % secs]), flush=True)
        os.environ.pop("RVCMI_RMVPE_UNET", None)
        res["rmvpe_on_device"] = f0
        if a.parity:
            par = []
            for B, T, seed in [(1, 32, 20240), (1, 64, 95), (2, 96, 127), (1, 1024, 1055)]:
                s = uc.seeded_weights(keys, seed)
                mel = uc.seeded_mel(B, T, 100 + T)
                ref = uc.forward(s, mel)
                h = rvc_amd.UNetHIP.from_state_dict(s, dev)
                got = h(mel.to(dev).transpose(-1, -2).unsqueeze(1)).transpose(1, 2).flatten(-2).cpu()
                half = uc.forward(uc.to(s, dev, torch.float16), mel.to(dev).half()).float().cpu()

                def err(v):
                    e = v.double() - ref.double()
                    return float(e.pow(2).mean().sqrt()), float(e.abs().max())

                (r_, m_), (hr, hm) = err(got), err(half)
                par.append(dict(B=B, T=T, ref_rms=float(ref.pow(2).mean().sqrt()), hip_rms=r_, hip_max=m_, torch_half_rms=hr, torch_half_max=hm,
                                rms_ratio=r_ / hr, max_ratio=m_ / hm))
                print(json.dumps(par[-1]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.parity)), exist_ok=True)
            json.dump(dict(reference="tests/unet_cases.forward, fp32, CPU", cases=par), open(a.parity, "w"), indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
