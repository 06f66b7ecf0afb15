"""fp64 restatement of the RMVPE deep U-Net and its head (``cnn(unet(x))``) with the rounding points of csrc/unet.hip / csrc/unet_kernels.hpp and no
others, primitive by primitive.  torch on the CPU; nothing here is imported by the product.

The rounding points, as the kernels have them:
  * every convolution weight is packed as fp16 (``pack_conv`` / ``pack_up``); scale and shift stay float;
  * eval-mode BatchNorm is folded in double, ``s = g / sqrt(v + 1e-5)``, ``h = b - m * s``, each then rounded to float (``Loader::bn``);
  * the two layers with one input channel stage ``fp16(fmaf(x, in_scale, in_shift))`` inside the image and 0 outside (``k_unet_first``): the
    fmaf is ONE rounding to float, then one to fp16 -- restated as such in either arithmetic, it defines the operand;
  * a primitive's epilogue is ``fmaf(acc, scale, shift)``, ReLU, ``+ res``, then ONE fp16 store: ``t``, the shortcut ``s``, a unit's output, the
    upsampled tensor; the pool stores ``fp16(((a + b) + (c + d)) / 4)``;
  * the head writes fp32: no rounding.

``forward(sd, mel)`` evaluates the network; ``trace=True`` also returns one record per primitive -- its fp16 operands (x0, x1, res), float
weights, scale, shift, ReLU flag, the ``kind`` number ``rvcmi_unet_debug_op`` takes, the unrounded fp64 result ``y`` and the sum of magnitudes
``A = |scale| (|w| * |x|) + |shift| + |res|`` -- which is what a teacher-forced sweep feeds to the kernel one primitive at a time
(``eval_prim(record, ...)`` evaluates one such record on the CPU).

  * ``arith="f32"``: the same thing in float32 -- the floor a correct fp32-accumulating kernel may sit at;
  * ``perturb={"seed": n, "split": bool}``: the K dimension summed the way the kernel may: (tap, 32-channel chunk) terms one after the other in a
    permuted order, with ``split`` cut into the slices ``forward_ksplit`` (the forward's own rule, restated) gives and the slices added in order;
  * ``rounded=False``: no rounding anywhere: the function torch computes (tests/unet_cases.forward) in fp64;
  * ``wrong=``: a named WRONG network (``WRONG``), each a mistake a kernel of this kind can make.
"""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
# the `kind` of rvcmi_unet_debug_op
K_3X3, K_1X1, K_UP, K_POOL, K_FIRST3, K_FIRST1, K_HEAD = 0, 1, 2, 3, 4, 5, 6

WRONG = ("res_before_relu",      # relu(bn(conv) + res) instead of relu(bn(conv)) + res
         "double_round",         # fp16(fp16(relu(bn(conv))) + res): the epilogue rounds before the residual and again after
         "scale_folded",         # the BatchNorm scale multiplied into the weights BEFORE they are rounded to fp16
         "shortcut_unrounded",   # the 1x1 shortcut added without its fp16 store
         "bias_dropped",         # the shortcut's bias left out
         "concat_swapped",       # cat(skip, upsampled) instead of cat(upsampled, skip)
         "up_flip",              # the transposed convolution's kernel indices 0 and 2 exchanged
         "pad_leak",             # the input BatchNorm's shift in place of the first convolution's zero padding
         "pool_pairwise")        # the pool's two pair sums rounded to fp16 before they are added


def r16(a):
    """Round to fp16, ONCE (torch converts double -> half through float, which rounds twice; numpy converts directly)."""
    if a.dtype == torch.float64:
        return torch.from_numpy(a.contiguous().numpy().astype(np.float16).astype(np.float64))
    return a.to(torch.float16).to(a.dtype)


def r32(a):
    return a.to(torch.float32).to(a.dtype)


def forward_ksplit(kind, Cin, Cout, M):
    """The K split ``conv()`` of csrc/unet.hip chooses for a layer of M input pixels when none is forced (1: the fused epilogue)."""
    if kind not in (K_3X3, K_1X1, K_UP) or Cout % 16:
        return 1
    pix_blk, co_blk = (128, 16) if Cout <= 16 else (128, 32) if Cout <= 32 else (64, 64)
    blocks = -(-M // pix_blk) * -(-Cout // co_blk) * (4 if kind == K_UP else 1)
    ntaps = {K_3X3: 9, K_UP: 4, K_1X1: 1}[kind]
    if blocks >= 128:
        return 1
    return min(-(-256 // blocks), 32, max(1, ntaps * -(-Cin // 32) // 4))


def _terms_sum(terms, ksplit, rng, like):
    """``terms``: callables in the kernel's K-loop order, each -> one (tap, chunk) term.  Slices as k_unet_conv cuts them, a permuted order
    inside a slice, the slices added in slice order (k_unet_reduce)."""
    n = len(terms)
    total = None
    for ks in range(ksplit):
        it0, it1 = ks * n // ksplit, (ks + 1) * n // ksplit
        acc = torch.zeros_like(like)
        for it in it0 + rng.permutation(it1 - it0):
            acc = acc + terms[it]()
        total = acc if total is None else total + acc
    return total


def conv_sum(x, w, kind, perturb=None, rng=None):
    """The convolution's sum alone, in x's dtype.  x [B, Cin, H, W]; w torch's [Cout, Cin, k, k], for ``K_UP`` ConvTranspose2d's
    [Cin, Cout, 3, 3] (stride 2, padding 1, output_padding 1).  Without ``perturb`` torch's own convolution; with it the sum term by term,
    the transposed convolution as the four output phases of unet_kernels.hpp (out[2y + 1] = in[y + 1] w[0] + in[y] w[2], out[2y] = in[y] w[1])."""
    up = kind == K_UP
    if perturb is None:
        if up:
            return F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
        return F.conv2d(x, w, padding=w.shape[-1] // 2)
    B, Cin, H, W = x.shape
    Cout = w.shape[1] if up else w.shape[0]
    chunks = [(c, min(c + 32, Cin)) for c in range(0, Cin, 32)]
    ksplit = forward_ksplit(kind, Cin, Cout, B * H * W) if perturb.get("split") else 1
    if not up:
        k = w.shape[-1]
        xp = F.pad(x, (k // 2,) * 4)

        def term(ky, kx, c0, c1):
            return lambda: F.conv2d(xp[:, c0:c1, ky:ky + H, kx:kx + W], w[:, c0:c1, ky:ky + 1, kx:kx + 1])

        terms = [term(ky, kx, c0, c1) for ky in range(k) for kx in range(k) for c0, c1 in chunks]
        return _terms_sum(terms, ksplit, rng, x.new_zeros(B, Cout, H, W))
    xp = F.pad(x, (0, 1, 0, 1))
    out = x.new_zeros(B, Cout, 2 * H, 2 * W)

    def term_up(ky, dy, kx, dx, c0, c1):
        return lambda: F.conv2d(xp[:, c0:c1, dy:dy + H, dx:dx + W], w[c0:c1, :, ky, kx].t().contiguous()[:, :, None, None])

    for py in (0, 1):
        for px in (0, 1):
            ys = ((0, 1), (2, 0)) if py else ((1, 0),)  # (kernel index, input offset), in the kernel's tap order
            xs = ((0, 1), (2, 0)) if px else ((1, 0),)
            terms = [term_up(ky, dy, kx, dx, c0, c1) for ky, dy in ys for kx, dx in xs for c0, c1 in chunks]
            out[:, :, py::2, px::2] = _terms_sum(terms, ksplit, rng, x.new_zeros(B, Cout, H, W))
    return out


def staged(r, dt, rounded=True):
    """The first layers' operand: fp16(float(x * in_scale + in_shift)), the product and sum exact in double as in an fmaf."""
    v = r["x0"].double() * r["in_scale"] + r["in_shift"]
    return (r16(r32(v)) if rounded else v).to(dt)


def _bc(v, dt):
    return v.to(dt)[None, :, None, None]


def eval_prim(r, arith="f64", perturb=None, wrong=None, rounded=True, magnitudes=False):
    """One primitive from its record -> its UNROUNDED result in ``arith`` (``magnitudes``: -> A, see the module docstring)."""
    dt = torch.float64 if arith == "f64" else torch.float32
    rng = np.random.default_rng(perturb["seed"]) if perturb else None
    kind = r["kind"]
    if kind == K_POOL:
        x = r["x0"].to(dt)
        if magnitudes:
            x = x.abs()
        a, b, c, d = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
        if wrong == "pool_pairwise":
            return (r16(a + b) + r16(c + d)) * 0.25
        return ((a + b) + (c + d)) * 0.25
    w, scale, shift = r["w"], r["scale"], r["shift"]
    if wrong == "scale_folded" and r["bn"]:
        w = w * (scale[None, :, None, None] if kind == K_UP else scale[:, None, None, None])
        scale = torch.ones_like(scale)
    w = (w.half() if rounded else w).to(dt)
    if wrong == "up_flip" and kind == K_UP:
        w = w.flip(2, 3)  # (index 1 stays, 0 and 2 change places, along both axes)
    pad_value = None
    if kind in (K_FIRST3, K_FIRST1):
        x = staged(r, dt, rounded)
        if kind == K_FIRST3 and wrong == "pad_leak":
            pad_value = float(r16(r32(torch.tensor(float(r["in_shift"]), dtype=torch.float64))))
    elif r["x1"] is not None:
        x = torch.cat((r["x1"], r["x0"]) if wrong == "concat_swapped" else (r["x0"], r["x1"]), 1).to(dt)
    else:
        x = r["x0"].to(dt)
    if wrong == "bias_dropped" and r["name"].endswith(".shortcut"):
        shift = torch.zeros_like(shift)
    res = r["res"].to(dt) if r["res"] is not None else None
    if magnitudes:
        x, w, scale, shift, res = x.abs(), w.abs(), scale.abs(), shift.abs(), (res.abs() if res is not None else None)
    if pad_value is not None:
        acc = F.conv2d(F.pad(x, (1, 1, 1, 1), value=pad_value), w)
    else:
        acc = conv_sum(x, w, kind, perturb, rng)
    y = acc * _bc(scale, dt) + _bc(shift, dt)
    if magnitudes:
        return y + res if res is not None else y
    if wrong == "res_before_relu" and res is not None:
        return F.relu(y + res)
    if r["relu"]:
        y = F.relu(y)
    if res is not None:
        if wrong == "double_round":
            y = r16(y)
        y = y + res
    return y


def _count(sd, fmt):
    n = 0
    while fmt % n in sd:
        n += 1
    return n


def forward(sd, mel, arith="f64", rounded=True, perturb=None, wrong=None, trace=False):
    """mel [B, 128, T] -> {"out": [B, T, head * 128] (what E2E.forward hands to its fc), "skips": the encoder levels' outputs [B, C, H, W],
    "trace": the records, when asked for}, all in ``arith``'s dtype."""
    assert wrong is None or wrong in WRONG, wrong
    dt = torch.float64 if arith == "f64" else torch.float32
    rnd = r16 if rounded else (lambda a: a)
    rf = r32 if rounded else (lambda a: a)
    records = []
    seed = [perturb["seed"] if perturb else 0]

    def bn(p):
        g, b, m, v = (sd[p + "." + k].double() for k in ("weight", "bias", "running_mean", "running_var"))
        s = g / torch.sqrt(v + BN_EPS)
        return rf(s), rf(b - m * s)

    def prim(name, kind, x0, x1=None, res=None, w=None, scale=None, shift=None, relu=0, bnp=None, in_scale=1.0, in_shift=0.0):
        if bnp is not None:
            scale, shift = bn(bnp)
        r = dict(name=name, kind=kind, x0=x0, x1=x1, res=res, w=w, scale=scale, shift=shift, relu=relu, bn=bnp is not None, in_scale=in_scale,
                 in_shift=in_shift)
        p = None
        if perturb:
            seed[0] += 1
            p = dict(perturb, seed=seed[0] * 7919)
        y = eval_prim(r, arith, p, wrong, rounded)
        if trace:
            r["y"] = y
            r["A"] = eval_prim(r, arith, None, None, rounded, magnitudes=True)
            for k in ("x0", "x1", "res", "w", "scale", "shift"):
                if r[k] is not None:
                    r[k] = r[k].float()  # (fp16 values, float weights, float-rounded scale and shift: all exact in float)
            records.append(r)
        return y

    def unit(p, x0, x1=None, first=None):
        f = dict(in_scale=first[0], in_shift=first[1]) if first else {}
        t = rnd(prim(p + ".conv.0", K_FIRST3 if first else K_3X3, x0, x1, w=sd[p + ".conv.0.weight"], relu=1, bnp=p + ".conv.1", **f))
        if p + ".shortcut.weight" in sd:
            b = sd[p + ".shortcut.bias"].double()
            s = prim(p + ".shortcut", K_FIRST1 if first else K_1X1, x0, x1, w=sd[p + ".shortcut.weight"], scale=torch.ones_like(b), shift=b, **f)
            if wrong != "shortcut_unrounded":
                s = rnd(s)
        else:
            s = x0
        return rnd(prim(p + ".conv.3", K_3X3, t, res=s, w=sd[p + ".conv.3.weight"], relu=1, bnp=p + ".conv.4"))

    levels = _count(sd, "unet.encoder.layers.%d.conv.0.conv.0.weight")
    blocks = _count(sd, "unet.encoder.layers.0.conv.%d.conv.0.weight")
    inters = _count(sd, "unet.intermediate.layers.%d.conv.0.conv.0.weight")
    x = mel.transpose(-1, -2).unsqueeze(1).contiguous()
    x = x.float() if rounded else x.to(dt)  # (the kernel takes the mel as float)
    s0, h0 = bn("unet.encoder.bn")
    skips = []
    for l in range(levels):
        for u in range(blocks):
            x = unit("unet.encoder.layers.%d.conv.%d" % (l, u), x, first=(float(s0), float(h0)) if l == 0 and u == 0 else None)
        skips.append(x)
        x = rnd(prim("unet.encoder.layers.%d.pool" % l, K_POOL, x))
    for i in range(inters):
        for u in range(blocks):
            x = unit("unet.intermediate.layers.%d.conv.%d" % (i, u), x)
    for i in range(levels):
        p = "unet.decoder.layers.%d" % i
        x = rnd(prim(p + ".conv1.0", K_UP, x, w=sd[p + ".conv1.0.weight"], relu=1, bnp=p + ".conv1.1"))
        for u in range(blocks):
            x = unit(p + ".conv2.%d" % u, x, skips[-1 - i] if u == 0 else None)
    b = sd["cnn.bias"].double()
    y = prim("cnn", K_HEAD, x, w=sd["cnn.weight"], scale=torch.ones_like(b), shift=b)
    out = dict(out=y.transpose(1, 2).flatten(-2), skips=skips)
    if trace:
        out["trace"] = records
    return out
