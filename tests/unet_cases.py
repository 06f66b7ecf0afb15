"""Shared pieces of the RMVPE U-Net tests (tests/test_cpu_unet.py, tests/test_gpu_unet.py) and of tools/make_golden_unet.py, tools/unet_time.py:

  * ``key_list``: the ``unet.*`` / ``cnn.*`` state-dict keys with shapes of a deep U-Net of a given geometry (the full network's list is ALSO
    a fixture written from the real reference, tests/golden/rmvpe_unet_keys.json; the CPU test compares the two);
  * ``seeded_weights``: weights keyed by name and shape, one generator, in key order;
  * ``forward``: an own functional evaluation of ``cnn(unet(x))`` over such a state dict (``F.conv2d``, ``F.batch_norm``, ``F.avg_pool2d``,
    ``F.conv_transpose2d``), in whatever dtype / device the tensors have -- fp32 on the CPU it is the tests' reference, ``.half()`` on the GPU
    it is the path whose error sets the tolerance;
  * ``StandIn``: a module tree built generically from a key list, with the same ``state_dict()`` keys and ``unet`` / ``cnn`` children;
  * the cases and the derived bars csrc/unet.hip is held to against the fp16-operand fp64 oracle (oracle/unet_oracle.py), primitive by primitive
    and stage by stage, with the runners that put a record of the oracle's trace, or a whole case, on the GPU (second half of the file; also
    tools/unet_layer_parity.py).
"""
import functools
import json
import os

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
FULL = dict(levels=5, blocks=4, inters=4, base=16)


def golden_keys():
    with open(os.path.join(GOLDEN, "rmvpe_unet_keys.json")) as f:
        return [(k, tuple(s)) for k, s in json.load(f)]


def _bn(p, c):
    return [(p + "." + k, (c,)) for k in ("weight", "bias", "running_mean", "running_var")] + [(p + ".num_batches_tracked", ())]


def _unit(p, cin, cout):
    out = [(p + ".conv.0.weight", (cout, cin, 3, 3))] + _bn(p + ".conv.1", cout) + [(p + ".conv.3.weight", (cout, cout, 3, 3))] + _bn(p + ".conv.4", cout)
    if cin != cout:
        out += [(p + ".shortcut.weight", (cout, cin, 1, 1)), (p + ".shortcut.bias", (cout,))]
    return out


def key_list(levels=5, blocks=4, inters=4, base=16, head=3):
    out = _bn("unet.encoder.bn", 1)
    cin, cout = 1, base
    for l in range(levels):
        for u in range(blocks):
            out += _unit("unet.encoder.layers.%d.conv.%d" % (l, u), cout if u else cin, cout)
        cin, cout = cout, 2 * cout
    for i in range(inters):
        for u in range(blocks):
            out += _unit("unet.intermediate.layers.%d.conv.%d" % (i, u), cout if (i or u) else cin, cout)
    cin = cout
    for i in range(levels):
        cout = cin // 2
        out += [("unet.decoder.layers.%d.conv1.0.weight" % i, (cin, cout, 3, 3))] + _bn("unet.decoder.layers.%d.conv1.1" % i, cout)
        for u in range(blocks):
            out += _unit("unet.decoder.layers.%d.conv2.%d" % (i, u), cout if u else 2 * cout, cout)
        cin = cout
    return out + [("cnn.weight", (head, base, 3, 3)), ("cnn.bias", (head,))]


def seeded_weights(keys, seed):
    """Convolutions uniform +-1/sqrt(fan_in); BatchNorm weight U[1.0, 1.4], bias 0.2 N(0,1), running mean 0.1 N(0,1), running variance
    U[0.3, 0.7]; shortcut / head biases 0.05 N(0,1).  With these gains every unit's convolution branch stays a visible fraction of its shortcut
    path and nothing leaves fp16's range through the 56 residual units (test_cpu_unet.py asserts both on the fp32 evaluation)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in keys:
        leaf = k.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            sd[k] = torch.zeros((), dtype=torch.int64)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            if ".conv1.0." in k:  # ConvTranspose2d [Cin, Cout, 3, 3], stride 2: an output pixel sums 9/4 taps of Cin on average
                fan_in = shape[0] * 9 / 4.0
            sd[k] = (2 * torch.rand(shape, generator=g) - 1) / fan_in ** 0.5
        elif leaf == "running_var":
            sd[k] = 0.3 + 0.4 * torch.rand(shape, generator=g)
        elif leaf == "running_mean":
            sd[k] = 0.1 * torch.randn(shape, generator=g)
        elif leaf == "weight":
            sd[k] = 1.0 + 0.4 * torch.rand(shape, generator=g)
        elif ".shortcut." in k or k == "cnn.bias":
            sd[k] = 0.05 * torch.randn(shape, generator=g)
        else:
            sd[k] = 0.2 * torch.randn(shape, generator=g)
    return sd


def seeded_mel(B, T, seed):
    """[B, 128, T] log-mel-like input (what ``E2E.forward`` takes)."""
    return 2 * torch.randn(B, 128, T, generator=torch.Generator().manual_seed(seed)) - 4


def _batch_norm(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)


def _res_unit(sd, p, x, stats):
    t = F.relu(_batch_norm(sd, p + ".conv.1", F.conv2d(x, sd[p + ".conv.0.weight"], padding=1)))
    t = F.relu(_batch_norm(sd, p + ".conv.4", F.conv2d(t, sd[p + ".conv.3.weight"], padding=1)))
    s = F.conv2d(x, sd[p + ".shortcut.weight"], sd[p + ".shortcut.bias"]) if p + ".shortcut.weight" in sd else x
    y = t + s
    if stats is not None:
        stats.append(dict(unit=p, branch_rms=float(t.float().pow(2).mean().sqrt()), shortcut_rms=float(s.float().pow(2).mean().sqrt()),
                          max_abs=float(max(t.float().abs().max(), s.float().abs().max(), y.float().abs().max()))))
    return y


def _count(sd, fmt):
    n = 0
    while fmt % n in sd:
        n += 1
    return n


def unet_forward(sd, x, pool=(2, 2), stats=None):
    """``DeepUnet.forward``: [B, 1, T, 128] -> [B, base, T, 128]."""
    levels = _count(sd, "unet.encoder.layers.%d.conv.0.conv.0.weight")
    blocks = _count(sd, "unet.encoder.layers.0.conv.%d.conv.0.weight")
    inters = _count(sd, "unet.intermediate.layers.%d.conv.0.conv.0.weight")
    x = _batch_norm(sd, "unet.encoder.bn", x)
    skips = []
    for l in range(levels):
        for u in range(blocks):
            x = _res_unit(sd, "unet.encoder.layers.%d.conv.%d" % (l, u), x, stats)
        skips.append(x)
        x = F.avg_pool2d(x, pool)
    for i in range(inters):
        for u in range(blocks):
            x = _res_unit(sd, "unet.intermediate.layers.%d.conv.%d" % (i, u), x, stats)
    for i in range(levels):
        p = "unet.decoder.layers.%d" % i
        x = F.conv_transpose2d(x, sd[p + ".conv1.0.weight"], stride=pool, padding=1, output_padding=(pool[0] - 1, pool[1] - 1))
        x = F.relu(_batch_norm(sd, p + ".conv1.1", x))
        x = torch.cat((x, skips[-1 - i]), dim=1)
        for u in range(blocks):
            x = _res_unit(sd, p + ".conv2.%d" % u, x, stats)
    return x


def head_forward(sd, x):
    return F.conv2d(x, sd["cnn.weight"], sd["cnn.bias"], padding=1)


def forward(sd, mel, stats=None):
    """What ``E2E.forward`` computes in front of its ``fc``: mel [B, 128, T] -> [B, T, 3 * 128]."""
    x = mel.transpose(-1, -2).unsqueeze(1)
    return head_forward(sd, unet_forward(sd, x, stats=stats)).transpose(1, 2).flatten(-2)


def to(sd, device=None, dtype=None):
    return {k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device=device)) for k, v in sd.items()}


class _Node(torch.nn.Module):
    pass


def _grow(root, keys, sd):
    for k, shape in keys:
        parts = k.split(".")
        m = root
        for p in parts[:-1]:
            if p not in m._modules:
                m.add_module(p, _Node())
            m = m._modules[p]
        v = sd[k].clone() if sd is not None else torch.zeros(shape, dtype=torch.int64 if parts[-1] == "num_batches_tracked" else torch.float32)
        if parts[-1] in ("weight", "bias"):
            m.register_parameter(parts[-1], torch.nn.Parameter(v, requires_grad=False))
        else:
            m.register_buffer(parts[-1], v)


class _UNet(_Node):
    def __init__(self, pool):
        super().__init__()
        self.pool = torch.nn.AvgPool2d(kernel_size=pool)

    def forward(self, x):
        sd = {"unet." + k: v for k, v in self.state_dict().items()}
        return unet_forward(sd, x, pool=tuple(self.pool.kernel_size))


class _Head(_Node):
    def forward(self, x):
        return F.conv2d(x, self.weight, self.bias, padding=1)


def _grow_real(root, keys, sd, pool):
    """The same tree with real ``torch.nn`` leaves (Conv2d, BatchNorm2d, ConvTranspose2d), typed from the keys and shapes."""
    shapes = dict(keys)
    prefixes = []
    for k, _ in keys:
        p = k.rsplit(".", 1)[0]
        if p not in prefixes:
            prefixes.append(p)
    for p in prefixes:
        w = shapes[p + ".weight"]
        if p + ".running_mean" in shapes:
            leaf = torch.nn.BatchNorm2d(w[0], momentum=0.01)
        elif p.endswith(".conv1.0"):
            leaf = torch.nn.ConvTranspose2d(w[0], w[1], (w[2], w[3]), stride=pool, padding=(1, 1), output_padding=(pool[0] - 1, pool[1] - 1), bias=False)
        else:
            leaf = torch.nn.Conv2d(w[1], w[0], (w[2], w[3]), padding=(w[2] // 2, w[3] // 2), bias=p + ".bias" in shapes)
        parts = p.split(".")
        m = root
        for q in parts[:-1]:
            if q not in m._modules:
                m.add_module(q, _Node())
            m = m._modules[q]
        m.add_module(parts[-1], leaf)
    # the reference's level containers remember their pooling as a plain attribute, None where a level does not pool: a recogniser that walks
    # ``modules()`` meets those too
    for name, m in root.named_modules():
        parts = name.split(".")
        if len(parts) == 4 and parts[2] == "layers" and parts[1] in ("encoder", "intermediate"):
            m.kernel_size = tuple(pool) if parts[1] == "encoder" else None
    if sd is not None:
        root.load_state_dict(sd, strict=True)


class StandIn(torch.nn.Module):
    """A module tree with exactly the keys of ``keys`` in its ``state_dict()``, ``unet`` and ``cnn`` children whose forward is the functional
    evaluator, and the forward of rvc/f0/e2e.py:44-46 up to (not including) ``fc``.  ``real_modules=True``: the leaves are real
    ``torch.nn.Conv2d`` / ``BatchNorm2d`` / ``ConvTranspose2d`` modules (what a recogniser that walks ``modules()`` meets in the real network)
    instead of bare parameter holders."""

    def __init__(self, keys, sd=None, pool=(2, 2), real_modules=False):
        super().__init__()
        self.unet = _UNet(pool)
        if real_modules:
            _grow_real(self, keys, sd, pool)
            assert isinstance(self.cnn, torch.nn.Conv2d)
        else:
            self.cnn = _Head()
            _grow(self, keys, sd)

    def forward(self, mel):
        mel = mel.transpose(-1, -2).unsqueeze(1)
        return self.cnn(self.unet(mel)).transpose(1, 2).flatten(-2)


# ---------------------------------------------------------------- the fp16-operand fp64 oracle (oracle/unet_oracle.py): cases and bars
#
# Nothing below is measured on the kernel.  tests/test_cpu_unet.py asserts every derivation and prints the ratios.
#
# Per primitive, teacher-forced (fed the oracle's own fp16 operands, so nothing has cascaded), for the unrounded fp64 value y:
#   * elementwise   |got - y| <= spacing16(max(|got|, |y|)) / 2 + GAMMA * A,   A = |scale| (|w| * |x|) + |shift| + |res| (the sum of magnitudes):
#     the one fp16 store of a value that fp32 accumulation has moved by at most GAMMA * A.  IEEE fp32 sums of the sweep's layers, in torch's order
#     and in the kernel's chunked / split order permuted, move y by at most 3.8e-7 A; 2^-19 is five times that, and at 2^-20 they still have no violation.  The head stores
#     fp32: its bound is GAMMA * A alone.
#   * flip share    at most FLIP_CAP of the elements differ from fp16(y).  The fp32 evaluations flip at most 2.2e-3 of a layer, an epilogue that
#     rounds twice flips at least 4.1e-2: 1e-2 is 4.5 times the one and a quarter of the other.
GAMMA = 2.0 ** -19
FLIP_CAP = 1e-2
SWEEP = (tuple(FULL.values()), 2, 32, 77)   # (levels, blocks, inters, base), B, T, seed: the deepest level is 1 x 4 pixels per item
SWEEP_CPU = (SWEEP, (tuple(FULL.values()), 1, 64, 78))
# the whole network and its stages: the full geometry, a reduced one with a batch, and base 48 (a first decoder unit reads 48 + 48 channels)
WHOLE = ((tuple(FULL.values()), 1, 32, 81), (tuple(FULL.values()), 2, 32, 82), ((3, 2, 2, 32), 2, 8, 83), ((1, 2, 1, 48), 1, 6, 84))


def case_id(c):
    return "%d-%d-%d-%d_B%d_T%d" % (c[0] + c[1:3])


def case_inputs(c):
    (levels, blocks, inters, base), B, T, seed = c
    return seeded_weights(key_list(levels, blocks, inters, base), seed), seeded_mel(B, T, 1000 + seed)


def spacing16(v):
    """the spacing of fp16 at |v|, elementwise (2^-24 below the normal range)"""
    e = torch.floor(torch.log2(v.abs().double().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def prim_check(got, rec, gamma=GAMMA):
    """``got``: a primitive's result [B, C, H, W] (the head's: fp32 values, any other's: fp16 values) against the record of the oracle's trace.
    -> {"flips": share of elements that are not fp16(y) (head: that leave the bound), "violations": elements outside the elementwise bound,
    "excess": the largest (|got - y| - spacing16 / 2) / A, i.e. how far fp32 accumulation must have moved y, "n"}."""
    from oracle import unet_oracle as uo

    y, A = rec["y"].double(), rec["A"].double()
    got = got.double()
    e = (got - y).abs()
    if rec["kind"] == uo.K_HEAD:
        half = torch.zeros_like(e)
        flips = float((e > gamma * A).double().mean())
    else:
        half = 0.5 * spacing16(torch.maximum(got.abs(), y.abs()))
        flips = float((got != uo.r16(y)).double().mean())
    tiny = torch.finfo(torch.float64).tiny
    return {"flips": flips, "violations": int((e > half + gamma * A).sum()), "excess": float(((e - half).clamp_min(0) / A.clamp_min(tiny)).max()),
            "n": got.numel()}


def skip_offsets(B, T, geometry):
    """Where ``run()`` of csrc/unet.hip leaves the encoder levels' outputs in the caller's workspace: after four full-size fp16 buffers, every
    part rounded up to 256 bytes.  -> ([(byte offset, (B, H, W, C)) per level], end)."""
    levels, base = geometry["levels"], geometry["base"]

    def up(n):
        return (n + 255) // 256 * 256

    off = 4 * up(B * T * 128 * base * 2)
    out = []
    for l in range(levels):
        shape = (B, T >> l, 128 >> l, base << l)
        out.append((off, shape))
        off += up(2 * shape[0] * shape[1] * shape[2] * shape[3])
    return out, off


def err(got, want):
    e = got.double() - want.double()
    return float(e.pow(2).mean().sqrt()), float(e.abs().max())


def ulp16(v):
    return float(spacing16(torch.tensor(float(v))))


def stages(res):
    """oracle result -> the tensors a forward leaves behind, by name: the skips (NCHW) and the head's output"""
    return dict([("skip%d" % l, s) for l, s in enumerate(res["skips"])] + [("out", res["out"])])


@functools.lru_cache(maxsize=None)
def sweep_trace(c=SWEEP):
    """The oracle's trace of a sweep case (computed once, never changed): one record per primitive."""
    from oracle import unet_oracle as uo

    sd, mel = case_inputs(c)
    with torch.no_grad():
        return tuple(uo.forward(sd, mel, trace=True)["trace"])


# The whole network and its stages (the five skip tensors a forward leaves in the caller's workspace, and the head's output) against the rounded
# oracle, in the form of tests/hubert_cases.py: bar = f * floor + additive, floor = the oracle in float32 against float64.  Here rounding flips
# cascade (the floor at the full network's output is 7e-3 RMS where y has RMS 8.4), so these bars see gross errors only.
#   * f: the perturbed fp32 evaluations (K summed in a permuted order, in chunks, in the forward's split slices; two seeds, every case of WHOLE)
#     moved the error against the fp64 oracle to at most 1.17 times the floor's RMS and 2.0 times its max-abs (a max-abs of one fp16 ulp
#     becoming two).  Twice that, rounded up to the next half: 2.5 and 4.
#   * additive: tests/hubert_cases.py measures it on the cases whose floor is 0.  No stage of WHOLE has one (test_cpu_unet.py asserts that, so
#     the term never carries a bar here); it is the smallest thing it can be, ONE flip of one element more than the floor saw:
#     ulp16(max |y|) for the max-abs, ulp16(max |y|) / sqrt(n) for the RMS.
# test_cpu_unet.py prints the ratios, asserts that the perturbed evaluations stay inside HALF of each bar and that the wrong variants that change
# values by more than a rounding stand clear of them.
F_RMS, F_MAX = 2.5, 4.0


def stage_bars(y32, y64):
    floor_rms, floor_max = err(y32, y64)
    one = ulp16(y64.abs().max())
    return {"floor_rms": floor_rms, "floor_max": floor_max, "bar_rms": F_RMS * floor_rms + one / y64.numel() ** 0.5, "bar_max": F_MAX * floor_max + one}


@functools.lru_cache(maxsize=None)
def whole_case(c):
    """-> {stage: {"y": the fp64 oracle's tensor, floor_*, bar_*}} of a case of WHOLE (computed once, never changed)"""
    from oracle import unet_oracle as uo

    sd, mel = case_inputs(c)
    with torch.no_grad():
        y64, y32 = stages(uo.forward(sd, mel)), stages(uo.forward(sd, mel, arith="f32"))
    return {k: dict(stage_bars(y32[k], y64[k]), y=y64[k]) for k in y64}


# ---------------------------------------------------------------- one primitive on the GPU

def _nhwc16(x, gpu):
    return x.permute(0, 2, 3, 1).contiguous().to(gpu, torch.float16)


def debug_op(gpu, kind, x0, x1, res, w, scale, shift, relu, cout, out_shape, ksplit=0, in_scale=1.0, in_shift=0.0, head=False):
    """One primitive through ``rvcmi_unet_debug_op``; tensors in torch's NCHW fp32 on the CPU -> the result as NCHW fp32 on the CPU."""
    import ctypes as C

    from rvc_amd import _lib

    B, _, H, W = x0.shape
    one = kind in (4, 5)
    d0 = x0[:, 0].contiguous().to(gpu) if one else _nhwc16(x0, gpu)
    d1 = _nhwc16(x1, gpu) if x1 is not None else None
    dr = _nhwc16(res, gpu) if res is not None else None
    if head:
        out = torch.full((B, H, cout, W), float("nan"), device=gpu, dtype=torch.float32)
    else:
        out = torch.full((out_shape[0], out_shape[2], out_shape[3], out_shape[1]), float("nan"), device=gpu, dtype=torch.float16)

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    wf = w.contiguous() if w is not None else None
    sc = scale.contiguous() if scale is not None else None
    sh = shift.contiguous() if shift is not None else None
    _lib.check(_lib.lib().rvcmi_unet_debug_op(kind, B, H, W, 1 if one else x0.shape[1], x1.shape[1] if x1 is not None else 0, cout, ptr(wf), ptr(sc), ptr(sh),
                                              int(relu), in_scale, in_shift, ptr(d0), ptr(d1), ptr(dr), ptr(out), ksplit, 0,
                                              C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
    torch.cuda.synchronize()
    o = out.cpu()
    return o.permute(0, 2, 1, 3).float() if head else o.permute(0, 3, 1, 2).float()


def run_record(gpu, rec, ksplit):
    """A record of the oracle's trace through ``rvcmi_unet_debug_op`` -> the kernel's result, NCHW on the CPU."""
    y = rec["y"]
    return debug_op(gpu, rec["kind"], rec["x0"], rec["x1"], rec["res"], rec["w"], rec["scale"], rec["shift"], rec["relu"], y.shape[1], y.shape, ksplit,
                    rec["in_scale"], rec["in_shift"], head=rec["kind"] == 6)


def run_whole(gpu, c):
    """``rvcmi_unet_forward`` with the caller's own workspace -> {stage: tensor on the CPU} as ``stages`` names them (skips NCHW)."""
    import rvc_amd
    from rvc_amd import _lib

    (levels, blocks, inters, base), B, T, _ = c
    sd, mel = case_inputs(c)
    hip = rvc_amd.UNetHIP.from_state_dict(sd, gpu)
    x = mel.transpose(-1, -2).contiguous().to(gpu)  # [B, T, 128] float
    nbytes = hip.workspace_bytes(B, T)
    offs, end = skip_offsets(B, T, dict(levels=levels, base=base))
    assert 0 < end <= nbytes, (end, nbytes)
    ws = torch.zeros(nbytes, device=gpu, dtype=torch.uint8)
    out = torch.full((B, T, hip.head_channels, 128), float("nan"), device=gpu)
    with torch.cuda.device(gpu):
        _lib.check(_lib.lib().rvcmi_unet_forward(hip._h, B, T, _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), _lib.stream_ptr(gpu)))
    torch.cuda.synchronize()
    got = {"out": out.cpu().flatten(-2)}
    for l, (off, shape) in enumerate(offs):
        n = 2 * shape[0] * shape[1] * shape[2] * shape[3]
        got["skip%d" % l] = ws[off:off + n].view(torch.float16).view(shape).permute(0, 3, 1, 2).float().cpu()
    return got
