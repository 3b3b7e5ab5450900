"""Per-layer reference for the native CenterNet forward: every engine op judged on its own.

The end-to-end parity tests compare the head output of a whole network with a golden file; a wrong
edge pixel in one of ~50 convolutions moves the head output by less than their tolerance. Here the
float64 oracle (oracle/ref_forward.py) runs with a hook at every boundary that is one engine op.
For each layer the hook

  (a) compares the oracle's value, computed from the layer's inputs *as the engine stored them*,
      with the tensor the engine stored for the op of that label (NativeEngine.op_outputs), and
  (b) returns the engine's tensor, so that the next layer is again judged on its own rounding only
      (teacher forcing).

A layer whose op stores nothing (it runs inside another op's launch) is not compared; the oracle's
value passes through and the next stored op is judged over the fused chain.

Layers. layer_graph() restates the engine's lowering (planner.cpp) from the state dict: every op is
`act(sum_seg conv(x_seg, w_seg) + bias [+ skip])` with the eval BatchNorm folded into
w_seg = w * gamma / sqrt(var + eps) per output channel (Engine::fold: folded in double, stored as
the compute dtype), or a ConvTranspose2d(k = s, stride s) + pad_to_match + skip. check() asserts for
every layer that this restatement and the oracle's own value agree to 1e-9, so the bounds below
always belong to the layer the oracle computed.

Bounds, per output element, in units of u = 2^-11 (fp16) or 2^-8 (bf16), the unit roundoff of the
compute dtype. With the absolute sum A = sum_seg conv(|x|, |w_seg|) (+ |skip| for the up-path add)
and its root-sum-square analogue Q = sqrt(sum_seg conv(x^2, w_seg^2)):

  deterministic   |got - ref| <= r u A + u |ref| + K 2^-24 A
  statistical     |got - ref| <= c u (|ref| + Q)

Derivation of the deterministic bound, for one output y = act(sum_k x_k w_k + b [+ skip]):
  * operands. The kernel multiplies x_k by fl(w_k) = w_k (1 + d_k), |d_k| <= u, and the products
    of two compute-dtype numbers are exact in the fp32 MFMA accumulator, so the sum moves by at most
    u sum |x_k| |w_k| = u A. Every further operand that was rounded to the compute dtype on the way
    and that the oracle sees unrounded adds one more u A, which gives r:
      - plain conv / conv + residual / root / heads with stored inputs: r = 1 (the weights);
      - the stem (stem.hip): its input is rounded too, the fp32 pixel or the u8 LUT entry is
        converted to the compute dtype when it is staged (stem.hip: `(T)__uint_as_float(raw)`,
        `lut[i] = (T)(...)`), and the oracle reads the fp32 image: r = 2. The separate staging
        launch (TV_STEM=0) stores the same rounded image, which the oracle does not read either;
      - block_layers.0.conv1 on stem_s2.hip: the stem's output is rounded to the compute dtype in
        LDS and never stored, behind it the staged image: r = 3. In that block's
        conv2+conv_residual only the 1x1 residual segment reads the stem (the samples stem_s2
        wrote: rounded, and not among the op outputs): r = 3 for that segment's part of A, r = 1
        for the 3x3 segment, whose input is stored (r u A is u sum_seg r_seg A_seg);
      - the 1x1 heads in the 3x3 heads' epilogue (conv3x3 EPI 1): the hidden layer is not stored,
        but it is not rounded to the compute dtype either: the epilogue feeds the second MFMA the
        fp32 activation v as a hi + lo pair (conv3x3_kernel.h: hi = T(v), lo = T(v - hi)), which
        leaves ~u^2 |v|. So the chain keeps r = 1 (the 1x1 weights), the tighter reading;
        HI_LO_UNSTORED lists that layer.
    In general, per segment, r = 1 + the number of unstored tensors rounded to the compute dtype
    between the segment and its nearest stored (or exact) input; check() counts them from which ops
    stored nothing.
  * accumulation. K products and the bias summed in fp32 in any order: at most K 2^-24 A (K = the
    reduction length, sum of cin * kh * kw over the segments; 2^-24 the fp32 unit roundoff).
  * activation. ReLU and LeakyReLU are 1-Lipschitz: the error does not grow.
  * output rounding. One rounding to the compute dtype: u |y|, dropped for fp32 outputs.
  * ConvTranspose2d(k = s, stride s) + pad_to_match + add (convt.hip): every output pixel is one
    phase's 1x1 conv over cin inputs (K = cin) plus the skip value, which is a stored input and
    enters exactly, but the sum u + skip is rounded once (the u |ref| term); |skip| is part of A so
    that the fp32 add of the skip is covered by the K 2^-24 A term.

The statistical bound treats the K operand roundings as independent: their sum has standard
deviation <= u Q / sqrt(3), the output rounding adds u |ref|. Its constant c is not derived but
measured on the CPU against the reference arithmetic only (emulate(): inputs as stored, folded
weights rounded to the compute dtype, fp32 accumulation, one output rounding) over every layer of
every case of tests/test_gpu_layers.py, and asserted at twice that maximum (C_STAT); the factor 2
covers another summation order and the extra roundings the statistical scale does not see: the
image the stem kernels round when they stage it (the emulated stem reads the fp32 image, as the
oracle does) and the unstored tensors of the fused chains.
tests/test_layer_ref_cpu.py re-measures C_MEASURED on every run.
"""
import numpy as np
import torch
import torch.nn.functional as F

import oracle
from oracle.ref_forward import HEADS_HIDDEN_LABEL, HEADS_OUT_LABEL, pad_to_match

# ("fp32": the operands are exact, u is the fp32 unit roundoff; used by tests/yolact_layer_ref.py on the
# routes the fp32 plan takes: its bound is K 2^-24 A + 2^-24 |ref|)
U = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp32": 2.0 ** -24}
TORCH_DTYPE = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
# Largest err / (u (|ref| + Q)) of the emulated reference arithmetic over every layer of every GPU
# case (test_layer_ref_cpu.test_emulation_within_bounds_and_measures_c), and the asserted constant
C_MEASURED = {"fp16": 1.96, "bf16": 2.31}
C_STAT = {p: 2.0 * v for p, v in C_MEASURED.items()}
IMG = "img"  # the network input's name among a layer's sources
STEM = "backbone.dla_down.projection_layer.0"
HI_LO_UNSTORED = {HEADS_HIDDEN_LABEL}  # unstored, yet carried at ~fp32: adds nothing to r


class Layer:
    """One engine op. kind "conv": segs = [(source label, folded weight [N, cin, kh, kw], stride,
    pad)], bias [N], act 0 none / 1 ReLU / 2 LeakyReLU(0.01). kind "convt": one seg (source, weight
    [cin, N, s, s], s, 0), bias, skip = label of the tensor added after pad_to_match."""

    def __init__(self, label, kind, segs, bias, act=0, skip=None, out_f32=False, K=None):
        self.label, self.kind, self.segs, self.bias, self.act = label, kind, segs, bias, act
        self.skip, self.out_f32 = skip, out_f32
        self.K = K if K is not None else sum(w.shape[1] * w.shape[2] * w.shape[3] for _, w, _, _ in segs)

    def sources(self):
        return [s for s, _, _, _ in self.segs] + ([self.skip] if self.skip else [])


def _fold(sd, conv, bn, ci0=0, cin=None):
    """Engine::fold: (folded weight, shift) of conv (+ eval BatchNorm), in float64."""
    w = sd[conv + ".weight"].double()
    w = w[:, ci0:ci0 + (cin if cin is not None else w.shape[1])]
    b = sd[conv + ".bias"].double()
    if bn is None:
        return w, b
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
    return w * s.view(-1, 1, 1, 1), (b - sd[bn + ".running_mean"].double()) * s + sd[bn + ".bias"].double()


def layer_graph(sd, heights, downsamples, prefix="backbone"):
    """The engine's ops (planner.cpp's forward lowering) in plan order: {label: Layer}."""
    layers = {}

    def add(layer):
        assert layer.label not in layers, layer.label
        layers[layer.label] = layer
        return layer.label

    def conv_bn_relu(p_conv, p_bn, src, stride, pad):
        w, b = _fold(sd, p_conv, p_bn)
        return add(Layer(p_conv, "conv", [(src, w, stride, pad)], b, 1))

    def block(p, x, stride):
        t = conv_bn_relu(p + ".conv1", p + ".bn1", x, stride, 1)
        w2, b2 = _fold(sd, p + ".conv2", p + ".bn2")
        wr, br = _fold(sd, p + ".conv_residual", p + ".bn_residual")
        return add(Layer(p + ".conv2+conv_residual", "conv", [(t, w2, 1, 1), (x, wr, stride, 0)], b2 + br, 1))

    def tree(p, x, h, stride, kids):
        if h == 1:
            left = block(p + ".tree_l", x, stride)
            right = block(p + ".tree_r", left, 1)
            kids = kids + [left, right]
            segs, off = [], 0
            for k in kids:
                c = layers[k].bias.numel()
                w, b = _fold(sd, p + ".root.conv", p + ".root.bn", off, c)
                segs.append((k, w, 1, 0))
                off += c
            return add(Layer(p + ".root.conv", "conv", segs, b, 1))
        left = tree(p + ".tree_l", x, h - 1, stride, [])
        return tree(p + ".tree_r", left, h - 1, 1, kids + [left])

    def up_add(p, j, x, skip):
        pr = conv_bn_relu(f"{p}.projection_layers.{j}.0", f"{p}.projection_layers.{j}.1", x, 1, 1)
        w = sd[f"{p}.upsample_layers.{j}.weight"].double()
        u = add(Layer(f"{p}.upsample_layers.{j}+pad_to_match+add", "convt", [(pr, w, w.shape[2], 0)],
                      sd[f"{p}.upsample_layers.{j}.bias"].double(), 0, skip=skip, K=w.shape[0]))
        return conv_bn_relu(f"{p}.output_layers.{j}.0", f"{p}.output_layers.{j}.1", u, 1, 1)

    dd = prefix + ".dla_down"
    x = conv_bn_relu(dd + ".projection_layer.0", dd + ".projection_layer.1", IMG, 1, 3)
    for i in range(downsamples):
        x = block(f"{dd}.block_layers.{i}", x, 2)
    feats = [x]
    for i, h in enumerate(heights):
        x = tree(f"{dd}.tree_layers.{i}", x, h, 2, [])
        feats.append(x)
    collected = []
    for i in range(len(feats) - 1):
        p = f"{prefix}.multi_ida_up.ida_up_layers.{i}"
        cur, outs = feats[-1], []
        for j in reversed(range(len(feats) - 1)):
            cur = up_add(p, j, cur, feats[j])
            outs.append(cur)
        feats = outs[::-1]
        collected.append(feats[-1])
    collected = collected[::-1]
    cur = collected[0]
    for i in range(len(collected) - 1):
        cur = up_add(prefix + ".ida_up_reverse", i, collected[i + 1], cur)
    n = 0
    while f"heads.{n}.0.weight" in sd:
        n += 1
    if n:
        w1 = torch.cat([sd[f"heads.{k}.0.weight"].double() for k in range(n)], 0)
        b1 = torch.cat([sd[f"heads.{k}.0.bias"].double() for k in range(n)], 0)
        hid = add(Layer(HEADS_HIDDEN_LABEL, "conv", [(cur, w1, 1, 1)], b1, 2))
        w2s = [sd[f"heads.{k}.2.weight"].double() for k in range(n)]
        hc = w2s[0].shape[1]
        w2 = torch.zeros((sum(w.shape[0] for w in w2s), n * hc, 1, 1), dtype=torch.float64)
        r0 = 0
        for k, w in enumerate(w2s):  # block diagonal: head k reads its own hidden channels
            w2[r0:r0 + w.shape[0], k * hc:(k + 1) * hc] = w
            r0 += w.shape[0]
        b2 = torch.cat([sd[f"heads.{k}.2.bias"].double() for k in range(n)], 0)
        add(Layer(HEADS_OUT_LABEL, "conv", [(hid, w2, 1, 0)], b2, 0, out_f32=True, K=hc))
    return layers


def _act(y, act):
    return F.relu(y) if act == 1 else F.leaky_relu(y, 0.01) if act == 2 else y


def _linear(layer, xs, fx=lambda t: t, fw=lambda t: t, bias=None):
    """sum_seg conv(fx(x), fw(w)) (+ bias), a ConvTranspose padded / cropped onto its target."""
    if layer.kind == "convt":
        src, w, s, _ = layer.segs[0]
        u = F.conv_transpose2d(fx(xs[src]), fw(w), bias, stride=s)
        return pad_to_match(u, xs[layer.skip].shape)
    y = None
    for src, w, stride, pad in layer.segs:
        t = F.conv2d(fx(xs[src]), fw(w), None, stride, pad)
        y = t if y is None else y + t
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def evaluate(layer, xs):
    """The layer in the dtype of its inputs (float64: the reference)."""
    y = _linear(layer, xs, bias=layer.bias.to(next(iter(xs.values())).dtype))
    if layer.kind == "convt":
        # the bias belongs to the ConvTranspose: none on the margin pad_to_match filled with zeros
        return y + xs[layer.skip]
    return _act(y, layer.act)


def abs_sums(layer, xs, weight=None):
    """(A, Q) of the module docstring; weight = {source label: factor of that source's part of A}
    gives sum_seg weight_seg conv(|x|, |w_seg|) (+ weight_skip |skip|) instead of A."""
    wt = weight or {}
    A = None
    for seg in layer.segs:
        one = Layer(layer.label, layer.kind, [seg], layer.bias, layer.act, layer.skip, layer.out_f32, layer.K)
        t = wt.get(seg[0], 1) * _linear(one, xs, torch.abs, torch.abs)
        A = t if A is None else A + t
    Q = torch.sqrt(_linear(layer, xs, torch.square, torch.square))
    if layer.kind == "convt":
        A = A + wt.get(layer.skip, 1) * xs[layer.skip].abs()
    return A, Q


def emulate(layer, xs, precision, weight_fault=None):
    """The reference arithmetic of a correct kernel: inputs as stored, folded weights rounded to the
    compute dtype, fp32 accumulation, one rounding of the output (none for fp32 outputs); float64
    result. weight_fault(seg index, rounded weight) -> weight lets a test break it."""
    dt = TORCH_DTYPE[precision]
    segs = []
    for i, (src, w, stride, pad) in enumerate(layer.segs):
        wr = w.float().to(dt).float()  # (pack_op_host: folded in double, staged as fp32, stored as dt)
        segs.append((src, wr if weight_fault is None else weight_fault(i, wr), stride, pad))
    low = Layer(layer.label, layer.kind, segs, layer.bias.float(), layer.act, layer.skip, layer.out_f32, layer.K)
    y = evaluate(low, {k: v.float() for k, v in xs.items() if k in layer.sources()})
    return (y if layer.out_f32 else y.to(dt)).double()


def bounds(layer, xs, ref, precision, r=1):
    """(deterministic bound, statistical scale u (|ref| + Q)) per element. r: one number, or
    {source label: r of the segment that reads it}: only a segment whose input has unstored rounded
    tensors behind it carries them (r u A becomes u sum_seg r_seg A_seg)."""
    u = U[precision]
    A, Q = abs_sums(layer, xs)
    rA = abs_sums(layer, xs, r)[0] if isinstance(r, dict) else r * A
    det = u * rA + layer.K * 2.0 ** -24 * A
    if not layer.out_f32:
        det = det + u * ref.abs()
    return det, u * (ref.abs() + Q)


def ratios(got, ref, det, stat):
    """Per element err / bound for both bounds (0 / 0 = 0, x / 0 = inf)."""
    err = (got - ref).abs()

    def div(a, b):
        return torch.where(a == 0, torch.zeros_like(a), a / b.clamp_min(1e-300))
    return div(err, det), div(err, stat)


def tile_of(kernel, idx, layer, xs):
    """Where the output element idx = (b, channel, y, x) falls in the tile grid of the kernel that ran."""
    b, _, y, x = idx
    name = kernel.split("<", 1)[0]
    if name == "tv::c3::conv3x3":  # conv3x3<T, OutT, TW, ..., NW>: TW x (64 NW / TW) pixels per frame
        a = kernel.split("<", 1)[1].rstrip(">").split(", ")
        tw, nw = int(a[2]), int(a[-1])
        return f"tile row {y // (64 * nw // tw)} col {x // tw} of {tw}x{64 * nw // tw} tiles"
    if name in ("tv::c3s2::conv3x3s2", "tv::ss2::stem_s2"):  # TW = 32, TH = 16 output pixels per frame
        return f"tile row {y // 16} col {x // 32} of 32x16 tiles"
    if layer.kind == "convt":
        # convt.hip and the generic phase scatter tile the flattened B*h*w source pixels (32 / 128)
        src, w, s, _ = layer.segs[0]
        _, _, h, wd = xs[src].shape
        th, tw = xs[layer.skip].shape[2:]
        sx, sy = max(0, (h * s - th) // 2), max(0, (wd * s - tw) // 2)  # pad_to_match: the H excess pads W
        if y < sy or x < sx or (y - sy) // s >= h or (x - sx) // s >= wd:
            return "uncovered margin of the target (the skip tensor's copy)"
        m = (b * h + (y - sy) // s) * wd + (x - sx) // s
        per = 32 if name == "tv::convt::convt_add" else 128
        return (f"source pixel ({(y - sy) // s}, {(x - sx) // s}) phase ({(y - sy) % s}, {(x - sx) % s}), "
                f"tile {m // per} of {per} flattened source pixels")
    # conv_lat (64), conv_pipe (256), conv_igemm (128) tile the flattened B*H*W output pixels;
    # conv_burst and conv1x1_stream size their tiles per layer: the flattened pixel is what they share
    per = {"tv::lat::conv_lat": 64, "tv::pipe::conv_pipe": 256, "tv::conv_igemm": 128}.get(name)
    m = (b * got_hw(layer, xs)[0] + y) * got_hw(layer, xs)[1] + x
    return f"flattened output pixel {m}" + (f", tile {m // per} of {per} pixels" if per else "")


def got_hw(layer, xs):
    """(H, W) of a conv layer's output."""
    src, w, stride, pad = layer.segs[0]
    _, _, h, wd = xs[src].shape
    return (h + 2 * pad - w.shape[2]) // stride + 1, (wd + 2 * pad - w.shape[3]) // stride + 1


class LayerReport:
    def __init__(self):
        self.rows = []   # (label, kernel, r, max det ratio, max stat ratio, worst index by det ratio, its tile)
        self.skipped = []

    def worst(self):
        return (max((r[3] for r in self.rows), default=0.0), max((r[4] for r in self.rows), default=0.0))

    def failures(self, c):
        out = []
        for label, kernel, r, rd, rs, idx, tile in self.rows:
            if rd > 1.0 or rs > c:
                b, ch, y, x = idx
                out.append(f"{label} [{kernel}] r={r}: {rd:.3g} x deterministic bound, {rs:.3g} x u(|ref|+Q) "
                           f"(c = {c:.3g}); worst at (b={b}, y={y}, x={x}, channel={ch}), {tile}")
        return out


def check(sd, heights, downsamples, img, precision, stored, kernels=None):
    """Teacher-forced per-layer comparison. sd: float64 state dict; img: float64 NCHW input;
    stored: {label: float64 NCHW tensor the engine stored for that op, or None}. Returns a
    LayerReport with one row per stored layer."""
    layers = layer_graph(sd, heights, downsamples)
    missing = [k for k in layers if k not in stored]
    assert not missing, f"no engine op with the labels {missing}"
    vals = {IMG: img}
    # rounded tensors the oracle sees unrounded, behind each value: the staged image behind the
    # input, +1 for every layer that was computed but not stored
    hidden = {IMG: 1}
    rep = LayerReport()
    kernels = kernels or {}

    def hook(label, t):
        layer = layers[label]
        xs = {s: vals[s] for s in layer.sources()}
        mine = evaluate(layer, xs)
        assert t.shape == mine.shape and float((t - mine).abs().max()) <= 1e-9 * max(1.0, float(t.abs().max())), \
            f"{label}: layer_graph() and the oracle disagree"
        behind = max(hidden[s] for s in layer.sources())
        got = stored[label]
        if got is None:
            vals[label], hidden[label] = t, behind + (0 if label in HI_LO_UNSTORED else 1)
            rep.skipped.append(label)
            return t
        assert got.shape == t.shape, (label, tuple(got.shape), tuple(t.shape))
        r = 1 + behind  # (reported; the bound takes it per segment)
        det, stat = bounds(layer, xs, t, precision, {s: 1 + hidden[s] for s in layer.sources()})
        rd, rs = ratios(got, t, det, stat)
        k = int(torch.argmax(rd))
        idx = tuple(int(v) for v in np.unravel_index(k, tuple(rd.shape)))
        rep.rows.append((label, kernels.get(label, ""), r, float(rd.max()), float(rs.max()), idx,
                         tile_of(kernels.get(label, ""), idx, layer, xs)))
        vals[label], hidden[label] = got, 0
        return got

    with torch.no_grad():
        oracle.centernet_forward(sd, img, heights, downsamples, dict(keypoints=False), hook=hook)
    assert len(rep.rows) + len(rep.skipped) == len(layers)
    return rep


def emulated_forward(sd, heights, downsamples, img, precision):
    """The whole forward in the reference arithmetic, layer by layer (the CPU stand-in for the
    engine's stored tensors): {label: float64 NCHW tensor}. The stem reads the fp32 image as the
    oracle does: that the kernels round it when they stage it is one of the extra roundings left to
    the factor 2 of C_STAT, not part of the measured constant."""
    layers = layer_graph(sd, heights, downsamples)
    vals = {IMG: img.float().double()}
    for label, layer in layers.items():
        vals[label] = emulate(layer, vals, precision)
    del vals[IMG]
    return vals


def nchw64(t, channels=None):
    """An engine tensor (NHWC, any dtype, any device) as the oracle's float64 NCHW."""
    t = t.detach().to("cpu").double().permute(0, 3, 1, 2)
    return (t if channels is None else t[:, :channels]).contiguous()


HEIGHTS, DOWNSAMPLES, N_LABELS = [1, 1, 1], 2, 4


def make_model(channels, precision):
    """tv.Centernet(tv.DLABackbone([1, 1, 1], [C] * 4, 2), 4 plain labels) with its own seeded weights:
    (model on the CPU, float64 state dict for the oracle)."""
    import tauv_vision_amd as tv
    from recipe import seeded_state_dict
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(False, None), A(False, None), A(False, None), False, False,
                                             None) for i in range(N_LABELS)])
    model = tv.Centernet(tv.DLABackbone(HEIGHTS, [channels] * (len(HEIGHTS) + 1), DOWNSAMPLES), oc,
                         precision=precision)
    sd = seeded_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()])
    model.load_state_dict(sd)
    return model.eval(), {k: v.double() for k, v in sd.items() if v.dtype.is_floating_point}


def case_frames(in_h, in_w, batch):
    """(u8 NHWC frames, their normalised fp32 NCHW image) of a geometry case."""
    from recipe import seeded_u8_frames, normalize
    frames = seeded_u8_frames(batch, in_h, in_w, seed=in_h * 1000 + in_w)
    return frames, normalize(frames.permute(0, 3, 1, 2).float() / 255.0).contiguous()
