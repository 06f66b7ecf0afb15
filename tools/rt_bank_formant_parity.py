"""How far is the EXISTING ``net_g.infer`` at batch 3 with one shared ``return_length2``, followed by the existing per-row ``SincResample``,
from the same at batch 1?  The bar of the bank-against-solo comparisons of tests/test_gpu_rt_formant.py, measured on that test's own
inputs (tests/rt_formant_cases.py) with code the per-session formant shift does not touch: for every shift the tests use, ALL three
sessions are given that shift (so the batch has one ``return_length2``, the call the library served before), the operands come from the
single-stream ``RealtimeVC(formant_shift=f)`` per session, and the synthetic v2/48k ``net_g.infer`` (HIP front + generator, noise fixed per
session) is called once at batch 3 and three times at batch 1.  Writes profiles/rt_bank_formant_parity.json:

    batch3_vs_batch1["<shift>"]: return_length2, upp_res, max_abs = the largest |difference| over sessions and blocks,
                                 rms = the largest per-(session, block) RMS, on the operands of ``rt_bank_cases.vc_blocks()``
    batch3_vs_batch1_end_to_end_operands["<shift>"]: the same on what the solo ``rvc_infer_hip`` (stub feeders) hands to ``net_g.infer``

A test's bar for a session is TWICE the pair recorded for the session's shift (tests/rt_formant_cases.py recorded_bar says why); a
recorded (0, 0) means bit equality.

    python tools/rt_bank_formant_parity.py [--out profiles/rt_bank_formant_parity.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _dist(a, b):
    e = a.double() - b.double()
    return float(e.abs().max()), float(e.pow(2).mean().sqrt())


def _entry(shift, rl2, upp_res, rows):
    return dict(return_length2=rl2, upp_res=upp_res, max_abs=max(r["max_abs"] for r in rows), rms=max(r["rms"] for r in rows), rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_bank_formant_parity.json"))
    a = ap.parse_args()
    import rt_bank_cases as cases
    import rt_formant_cases as fc
    import rvc_amd
    from rvc_amd.realtime import rvc_infer_hip

    dev = torch.device("cuda:0")
    S = 3
    idx = cases.index_768()
    index = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=dev)
    net = cases.BankNet(dev, S)
    blocks = cases.vc_blocks(S, 2)
    first = {}
    for f in fc.FORMANTS:
        rl2, upp_res = fc.geometry(f)
        ops = fc.solo_operands(index, dev, blocks, [f] * S)
        rows = []
        for b in range(len(blocks)):
            batch = fc.direct_batch(net, ops[b], dev, rl2)
            for s in range(S):
                got = fc.solo_resample(batch[s], upp_res, dev)
                ref = fc.solo_resample(fc.direct_solo(net, ops[b][s], s, dev, rl2), upp_res, dev)
                mx, rms = _dist(got, ref)
                rows.append(dict(block=b, session=s, max_abs=mx, rms=rms, signal_rms=float(ref.double().pow(2).mean().sqrt())))
                print("shift %+.2f (return_length2 %d, upp_res %d) batch 3 vs 1: block %d session %d  max abs %.3e  rms %.3e" % (f, rl2, upp_res, b, s, mx, rms))
        first["%.2f" % f] = _entry(f, rl2, upp_res, rows)
    # the end-to-end test's operands: what the solo rvc_infer_hip hands to net_g.infer, stacked at batch 3
    seen = {}
    inner = net.infer

    def record(phone, lengths, sid, pitch=None, pitchf=None, **kw):
        seen.update(phone=phone.clone(), pitch=pitch.clone(), pitchf=pitchf.clone())
        return inner(phone, lengths, sid, pitch=pitch, pitchf=pitchf, **kw)

    second = {}
    for f in fc.E2E_FORMANTS:
        rl2, upp_res = fc.geometry(f)
        solos = [fc.e2e_solo_rvc(net, index, dev, fc.E2E_KEYS[s], f, []) for s in range(S)]
        rows = []
        for b, wav in enumerate(cases.e2e_waves(S, 2)):
            o, ref = [], []
            for s in range(S):
                net.rows = slice(s, s + 1)
                net.infer = record
                ref.append(rvc_infer_hip(solos[s], wav[s].to(dev), cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0))
                net.infer = inner
                o.append(dict(seen))
            batch = fc.direct_batch(net, o, dev, rl2, sids=[0, 0, 0])
            for s in range(S):
                mx, rms = _dist(fc.solo_resample(batch[s], upp_res, dev), ref[s])
                rows.append(dict(block=b, session=s, max_abs=mx, rms=rms))
                print("shift %+.2f (return_length2 %d, upp_res %d) batch 3 vs 1, end-to-end operands: block %d session %d  max abs %.3e  rms %.3e" % (
                    f, rl2, upp_res, b, s, mx, rms))
        second["%.2f" % f] = _entry(f, rl2, upp_res, rows)
    res = dict(device=torch.cuda.get_device_name(dev),
               what="net_g.infer (synthetic v2/48k, HIP front + generator, fp16 operands, noise fixed per session) with ONE return_length2 at batch 3 "
                    "+ the per-row SincResample(upp_res, 480) against the same at batch 1; T = 70, skip_head = 40, return_length = 20; all three "
                    "sessions at the entry's shift; operands of tests/rt_formant_cases.py prepared by the single-stream code",
               bar="a test's bar for a session is twice the (max_abs, rms) of the session's shift",
               batch3_vs_batch1=first, batch3_vs_batch1_end_to_end_operands=second)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
