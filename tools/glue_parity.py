"""The worst error per family of the glue's edge cases (tests/glue_cases.py, run by tests/test_gpu_glue_edges.py) from one MI355X run ->
profiles/glue_edges_parity.json.  These numbers are RECORDED, not asserted: the bars are the tests'.

    python tools/glue_parity.py [--out profiles/glue_edges_parity.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _f0(rows):
    rel, bins, zeros = 0.0, 0, 0
    for _, (pitch, pitchf), (want_p, want_f) in rows:
        rel = max(rel, float(np.max(np.abs(pitchf.astype(np.float64) - want_f) / np.maximum(np.abs(want_f), 1e-30), initial=0.0)))
        bins += int((pitch != want_p).sum())
        zeros += int(((pitchf == 0) != (want_f == 0)).sum())
    return dict(cases=len(rows), frames=int(sum(len(r[2][0]) for r in rows)), pitchf_max_rel=rel, pitch_bins_differing=bins, zero_set_differing=zeros)


def _exact(rows):
    a = [np.asarray(g) != np.asarray(w) for _, g, w in rows]
    return dict(cases=len(rows), values=int(sum(x.size for x in a)), values_differing=int(sum(x.sum() for x in a)))


def _rel(rows, atol):
    worst, where = 0.0, None
    for what, got, want in rows:
        e = np.abs(got.astype(np.float64) - want)
        rel = float(np.max(np.where(e <= atol, 0.0, e / np.maximum(np.abs(want), 1e-30))))
        if rel >= worst:
            worst, where = rel, what
    return dict(cases=len(rows), max_rel_above_atol=worst, atol=atol, worst_case=where, all_finite=bool(all(np.isfinite(g).all() for _, g, _ in rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glue_edges_parity.json"))
    a = ap.parse_args()
    import glue_cases as gc
    import test_gpu_glue_edges as t

    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(dev),
               what="worst observed error of the device-resident glue against oracle/glue_oracle.py on the edge cases of tests/glue_cases.py; "
                    "recorded, not asserted (bars: tests/glue_cases.py)")
    res["f0_rmvpe_patterns"] = _f0(t.run_rmvpe_patterns(dev))
    res["f0_post_patterns"] = _f0(t.run_post_patterns(dev))
    res["f0_decode_edges"] = _f0(t.run_decode_edges(dev))
    res["f0_lds_threshold"] = _f0(t.run_f0_thresholds(dev))
    res["expand_protect"] = _exact([(w, g.numpy(), x.numpy()) for w, g, x in t.run_expand(dev)])
    res["scale_int16_range"] = _exact(t.run_int16(dev))
    sola = t.run_sola(dev)
    res["sola"] = dict(cases=len(sola), offsets_differing=int(sum(g[2] != w[2] for _, g, w in sola)),
                       samples_differing=int(sum((g[0] != w[0]).sum() + (g[1] != w[1]).sum() for _, g, w in sola)))
    res["change_rms"] = _rel(t.run_change_rms(dev), gc.CHANGE_RMS_TOL["atol"])
    res["envelope_mix"] = _rel(t.run_envelope_mix(dev), gc.ENVELOPE_TOL["atol"])
    rs = t.run_resample(dev)
    res["sinc_resample"] = dict(cases=len(rs), max_abs_over_max1=max(float(np.abs(g - w).max() / max(1.0, np.abs(w).max())) for _, g, w in rs))
    pv = {}
    for n in gc.PV_EDGE_SIZES:
        for what, got, (r32, r64) in t.run_phase_vocoder(dev, n):
            r_dev, m_dev, r_32, m_32 = gc.pv_errors(got, r32, r64)
            pv[what] = dict(rms=r_dev, max_abs=m_dev, reference_fp32_rms=r_32, reference_fp32_max_abs=m_32)
    res["phase_vocoder"] = pv
    for k, v in res.items():
        print(k, json.dumps(v) if k != "phase_vocoder" else "")
    for k, v in pv.items():
        print("  %-16s rms %.2e max %.2e   (reference fp32: %.2e / %.2e)" % (k, v["rms"], v["max_abs"], v["reference_fp32_rms"], v["reference_fp32_max_abs"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
