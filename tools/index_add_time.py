"""Cost of growing an index on the device (``IVFFlatHIP.add`` = ``rvcmi_ivf_add``) and of the reference's index recipe (web.py:547-571:
train, then ``index.add`` in batches of 8192) against the one-shot build, for a 100k x 768 and a 1M x 256 training set (``nlist`` by the
reference's formula).  All legs run in one process, alternating after a warm-up of each; host wall clock around synchronised calls,
median and range of ``--reps`` repeats in ms:

  (a) add_host / add_device: ONE ``add`` of 8192 rows (numpy rows copied up once / a resident CUDA tensor) into the full index.  Every repeat
      starts from a handle that adopts the same blob (``from_blob``), which an add leaves untouched;
  (b) recipe_trained_plus_adds: ``IVFFlatHIP.trained(x)`` then ``add`` of 8192 rows at a time, rows on the host as in the reference;
  (c) one_shot_train: ``IVFFlatHIP.train(x)`` (``rvcmi_ivf_build``) of this tree;
  (d) one_shot_train_parent: the same call into a librvcmi.so built from the PARENT commit (``--parent-lib``; left out when not given).

(b), (c) and (d) must give the same index file, byte for byte.  Writes profiles/index_add_time.json.

    python tools/index_add_time.py [--reps 10] [--parent-lib /path/to/parent/librvcmi.so] [--out profiles/index_add_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import synth  # noqa: E402

BATCH = 8192


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3), "max_ms": round(float(np.max(ms)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--sizes", type=str, nargs="+", default=["100000x768", "1000000x256"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_add_time.json"))
    args = ap.parse_args()
    import rvc_amd
    from rvc_amd import _lib

    dev = torch.device("cuda:0")
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        sig = {name: (res, a) for name, res, a in _lib.SYMBOLS}
        for name in ("rvcmi_ivf_build", "rvcmi_ivf_write_file", "rvcmi_ivf_destroy", "rvcmi_last_error"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = sig[name]
    tmp = tempfile.mkdtemp()

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(dev)
        return r, (time.perf_counter() - t0) * 1e3

    def file_bytes(idx):
        path = os.path.join(tmp, "i.index")
        rvc_amd.write_index(idx, path)
        return open(path, "rb").read()

    rows = []
    for size in args.sizes:
        n, d = (int(v) for v in size.split("x"))
        x = synth.make_clustered_rows(n, d, max(8, n // 400), seed=n)
        nlist = max(1, min(int(16 * np.sqrt(n)), n // 39))
        extra = synth.make_clustered_rows(BATCH, d, max(8, n // 400), seed=n)  # the 8192 rows of leg (a): the same mixture
        extra_dev = torch.from_numpy(extra).to(dev)

        def one_shot():
            return rvc_amd.IVFFlatHIP.train(x, nlist=nlist, niter=args.niter, device=dev)

        def recipe():
            idx = rvc_amd.IVFFlatHIP.trained(x, nlist=nlist, niter=args.niter, device=dev)
            for i in range(0, n, BATCH):
                idx.add(x[i:i + BATCH])
            return idx

        def one_shot_parent():
            h = C.c_void_p(None)
            rc = parent.rvcmi_ivf_build(d, n, x.ctypes.data_as(C.c_void_p), nlist, args.niter, 1234, 0, C.c_void_p(None), C.byref(h))
            assert rc == 0, parent.rvcmi_last_error()
            return h

        base, _ = timed(one_shot)  # warm-up of each leg; the three builds agree
        want = file_bytes(base)
        assert file_bytes(timed(recipe)[0]) == want
        if parent is not None:
            h = timed(one_shot_parent)[0]
            path = os.path.join(tmp, "p.index")
            assert parent.rvcmi_ivf_write_file(h, path.encode()) == 0 and open(path, "rb").read() == want
            parent.rvcmi_ivf_destroy(h)
        blob = base.blob()
        del base

        def add_from(rows_):
            idx = rvc_amd.IVFFlatHIP.from_blob(blob)
            _, ms = timed(lambda: idx.add(rows_))
            assert idx.ntotal == n + BATCH
            return ms

        add_from(extra), add_from(extra_dev)
        t = {"add_host": [], "add_device": [], "recipe": [], "one_shot": [], "parent": []}
        for _ in range(args.reps):
            t["add_host"].append(add_from(extra))
            t["add_device"].append(add_from(extra_dev))
            t["recipe"].append(timed(recipe)[1])
            t["one_shot"].append(timed(one_shot)[1])
            if parent is not None:
                h, ms = timed(one_shot_parent)
                parent.rvcmi_ivf_destroy(h)
                t["parent"].append(ms)
        row = {"rows": n, "d": d, "nlist": nlist, "niter": args.niter, "blob_mib": round(blob.numel() / 2 ** 20, 1),
               "add_8192_from_host": stats(t["add_host"]), "add_8192_from_device": stats(t["add_device"]),
               "recipe_trained_plus_adds_of_8192": stats(t["recipe"]), "adds_in_recipe": (n + BATCH - 1) // BATCH,
               "one_shot_train": stats(t["one_shot"]), "one_shot_train_parent": stats(t["parent"]) if parent is not None else None}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del blob
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "host_threads": torch.get_num_threads(),
           "note": "host wall clock around synchronised calls, legs alternating in one process after a warm-up of each; add_8192_*: one add into the "
                   "full index, each repeat from a handle adopting the same blob; recipe: IVFFlatHIP.trained + adds of 8192 host rows; one_shot_train: "
                   "IVFFlatHIP.train of this tree; one_shot_train_parent: rvcmi_ivf_build of a library built from the parent commit; the three builds "
                   "give byte-identical index files",
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
