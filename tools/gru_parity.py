"""csrc/gru.hip against the fp16-operand fp64 oracle (oracle/gru_oracle.py) over the case table of tests/gru_cases.py, once:

    python tools/gru_parity.py --out profiles/gru_parity.json

Per case: the noise floor (the oracle's recurrence in float32 against float64) and the bars derived from it, the error of
``rvcmi_gru_forward`` against the oracle and its ratios to the floor, and -- for context -- its error against ``torch.nn.GRU`` in fp32 on the
CPU, the comparison of tests/test_gpu_gru.py's first half.  The ragged entry is listed per sequence.  Needs a GPU.
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gru_cases as gc  # noqa: E402


def _record(name, y, b, y_torch):
    rms, mx = gc.err(y, b["y"])
    t_rms, t_max = gc.err(y, y_torch)
    rec = {"case": name, "floor_rms": b["floor_rms"], "floor_max": b["floor_max"], "bar_rms": b["bar_rms"], "bar_max": b["bar_max"],
           "hip_rms": rms, "hip_max": mx, "rms_ratio": rms / b["floor_rms"], "max_ratio": mx / b["floor_max"],
           "within_bars": bool(rms <= b["bar_rms"] and mx <= b["bar_max"]), "torch_fp32_rms": t_rms, "torch_fp32_max": t_max}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import rvc_amd
    from rvc_amd import _lib

    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def p(t):
        return C.c_void_p(t.data_ptr())

    cases = []
    for c in gc.TABLE:
        ref = gc.module(c)
        x = gc.inputs(c).half()
        with torch.no_grad():
            y_torch = ref(x.float())[0].numpy()
        m = rvc_amd.GRUHIP(ref, device=dev)
        xd = x.to(dev).contiguous()
        y = torch.empty(c.B, c.T, 512, device=dev)
        _lib.check(L.rvcmi_gru_forward(m._h, c.B, c.T, p(xd), p(y), None, st))
        torch.cuda.synchronize()
        cases.append(_record(gc.case_id(c), y.cpu().numpy(), gc.bars(c), y_torch))
    gru, x, off = gc.ragged_case()
    m = rvc_amd.GRUHIP(gru, device=dev)
    xd = x.half().to(dev).contiguous()
    off_d = torch.tensor(off, dtype=torch.int32, device=dev)
    y = torch.empty(off[-1], 512, device=dev)
    _lib.check(L.rvcmi_gru_forward_ragged(m._h, len(off) - 1, (C.c_int * len(off))(*off), p(off_d), p(xd), p(y), None, st))
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    ragged = []
    for i, b in enumerate(gc.ragged_bars()):
        with torch.no_grad():
            y_torch = gru(x[off[i]: off[i + 1]].half().float()[None])[0][0].numpy()
        ragged.append(_record("ragged T%d" % (off[i + 1] - off[i]), y[off[i]: off[i + 1]], b, y_torch))
    out = {"reference": "oracle/gru_oracle.bigru, float64, fp16 operands (x, W_ih, W_hh, the copy of h in W_hh . h)",
           "floor": "the same recurrence in float32 against float64; bar_rms = 3 * floor_rms + 1e-6, bar_max = 4 * floor_max + 4e-6",
           "cases": cases, "ragged": ragged}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
