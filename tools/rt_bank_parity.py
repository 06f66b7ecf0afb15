"""How far is the EXISTING ``net_g.infer`` at batch 3 from batch 1?  The bar of the bank-against-solo comparisons of
tests/test_gpu_rt_bank.py, measured on that test's own inputs (tests/rt_bank_cases.py) with code the realtime bank does not touch:
the operands come from the single-stream ``RealtimeVC`` per session, and the synthetic v2/48k ``net_g.infer`` (HIP front + generator,
noise fixed per session) is called once at batch 3 and three times at batch 1.  Writes profiles/rt_bank_parity.json:

    batch3_vs_batch1: max_abs = the largest |difference| over sessions and blocks, rms = the largest per-(session, block) RMS

Both zero means the batched ``infer`` is batch-invariant on these inputs and the tests require bit equality; otherwise these two numbers
ARE the tests' bar (no margin: both sides of those tests run the same kernels on fixed inputs).  Also recorded, for information: the same
distance at batch 2 on the operands of the end-to-end test (stub feeders, two keys).

    python tools/rt_bank_parity.py [--out profiles/rt_bank_parity.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_bank_parity.json"))
    a = ap.parse_args()
    import rt_bank_cases as cases
    import rvc_amd
    from rvc_amd.realtime import rvc_infer_hip

    dev = torch.device("cuda:0")
    S = 3
    idx = cases.index_768()
    index = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=dev)
    net = cases.BankNet(dev, S)
    blocks = cases.vc_blocks(S, 2)
    ops = cases.solo_operands(net, index, dev, blocks)
    rows = []
    for b in range(len(blocks)):
        batch = cases.direct_batch(net, ops[b], dev)
        again = cases.direct_batch(net, ops[b], dev)
        for s in range(S):
            mx, rms = _dist(batch[s], cases.direct_solo(net, ops[b][s], s, dev))
            rows.append(dict(block=b, session=s, max_abs=mx, rms=rms, signal_rms=float(batch[s].double().pow(2).mean().sqrt()),
                             batch_repeatable=bool(torch.equal(batch[s], again[s]))))
            print("batch 3 vs 1: block %d session %d  max abs %.3e  rms %.3e" % (b, s, mx, rms))
    # the end-to-end test's operands: what the solo rvc_infer_hip hands to net_g.infer, stacked at batch 2
    seen = {}
    inner = net.infer

    def record(phone, lengths, sid, pitch=None, pitchf=None, **kw):
        seen.update(phone=phone.clone(), pitch=pitch.clone(), pitchf=pitchf.clone())
        return inner(phone, lengths, sid, pitch=pitch, pitchf=pitchf, **kw)

    rows2 = []
    solos = [cases.stub_rvc(net, index, dev, cases.E2E_KEYS[s]) for s in range(2)]
    for b, wav in enumerate(cases.e2e_waves(2, 2)):
        o, ref = [], []
        for s in range(2):
            net.rows = slice(s, s + 1)
            net.infer = record
            ref.append(rvc_infer_hip(solos[s], wav[s].to(dev), cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0))
            net.infer = inner
            o.append(dict(seen))
        batch = cases.direct_batch(net, o, dev, sids=[0, 0])
        for s in range(2):
            mx, rms = _dist(batch[s], ref[s])
            rows2.append(dict(block=b, session=s, max_abs=mx, rms=rms))
            print("batch 2 vs 1 (end-to-end operands): block %d session %d  max abs %.3e  rms %.3e" % (b, s, mx, rms))
    res = dict(device=torch.cuda.get_device_name(dev),
               what="net_g.infer (synthetic v2/48k, HIP front + generator, fp16 operands, noise fixed per session) at batch 3 against batch 1, "
                    "T = 70, skip_head = 40, return_length = 20, operands of tests/rt_bank_cases.py prepared by the single-stream RealtimeVC",
               batch3_vs_batch1=dict(max_abs=max(r["max_abs"] for r in rows), rms=max(r["rms"] for r in rows), rows=rows),
               batch2_vs_batch1_end_to_end_operands=dict(max_abs=max(r["max_abs"] for r in rows2), rms=max(r["rms"] for r in rows2), rows=rows2))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
