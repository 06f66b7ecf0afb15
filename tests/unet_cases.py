"""Shared pieces of the RMVPE U-Net tests (tests/test_cpu_unet.py, tests/test_gpu_unet.py) and of tools/make_golden_unet.py, tools/unet_time.py:

  * ``key_list``: the ``unet.*`` / ``cnn.*`` state-dict keys with shapes of a deep U-Net of a given geometry (the full network's list is ALSO
    a fixture written from the real reference, tests/golden/rmvpe_unet_keys.json; the CPU test compares the two);
  * ``seeded_weights``: weights keyed by name and shape, one generator, in key order;
  * ``forward``: an own functional evaluation of ``cnn(unet(x))`` over such a state dict (``F.conv2d``, ``F.batch_norm``, ``F.avg_pool2d``,
    ``F.conv_transpose2d``), in whatever dtype / device the tensors have -- fp32 on the CPU it is the tests' reference, ``.half()`` on the GPU
    it is the path whose error sets the tolerance;
  * ``StandIn``: a module tree built generically from a key list, with the same ``state_dict()`` keys and ``unet`` / ``cnn`` children.
"""
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
