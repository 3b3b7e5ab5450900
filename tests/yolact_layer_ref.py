"""Per-layer reference for the native YOLACT plans (TV_ARCH_RESNET18, TV_ARCH_YOLACT_HEAD, TV_ARCH_YOLACT):
the method of tests/layer_ref.py — every engine op judged on its own, from the tensors the engine stored
(teacher forcing), under a derived deterministic bound and a CPU-measured statistical one — applied to
the ops of csrc/planner_resnet.cpp, planner_yolact_head.cpp and planner_protonet.cpp.

resnet18_layers(), yolact_head_layers() and protonet_layers() restate those planners' lowering from a
reference-layout state dict: one Layer per engine op, in plan order, under the engine's op labels
(tv_engine_op_label). check() refuses a label the engine has and the graph lacks, or the reverse.
tests/test_yolact_layer_ref_cpu.py shows that the graph, evaluated in float64 without forcing, is
tests/resnet18_ref.py and tests/yolact_head_ref.py to 1e-9.

Notation as layer_ref: u the unit roundoff of the compute dtype (2^-11 fp16, 2^-8 bf16, 2^-24 fp32),
A = sum |x_k| |w_k|, Q = sqrt(sum x_k^2 w_k^2), K the reduction length, per output element

  deterministic   |got - ref| <= u sum_seg r_seg A_seg + K 2^-24 A + u |ref|        (+ P, below)
  statistical     |got - ref| <= c u (|ref| + Q)

Every rounding to the compute dtype is within max(u |x|, ETA) of x, ETA half the smallest subnormal
(2^-25 in fp16: a pixel or a sum below 2^-14 is rounded on the subnormal grid); wherever "u |ref|" or
"one rounding" stands below, ETA is added (the fp32 image and the seeded maps do hold such values).

Layer kinds and where their bounds come from (the kernel's text is named per kind):

 conv         layer_ref's conv, with three extensions.
              * identity K-segments (pack_op_host, `sg.identity`): the residual x enters the GEMM as
                a 1x1 segment whose weight is the unit matrix. Plain (ResNet `conv2 + bn2 + x`, the
                head Bottleneck's `conv3 + x`): the stored weight is exactly 1 in every dtype, the
                product x * 1 is exact: r_seg = 0, and the segment adds nothing to Q. Through an eval
                BatchNorm (the head block's last GEMM): pack_op_host stores `(float)scale[co]` rounded to
                the compute dtype on the diagonal and adds the shift to the fp32 bias: a weight like
                any other, r_seg = 1. Either way the segment's cin products are part of K and A (the
                kernel does run the k-steps, over zeros off the diagonal).
              * the 1x1 / stride-2 `downsample` of layerL.0 is a second segment with folded weights
                (r_seg = 1), read at stride 2 from the block's input.
              * out_f32 (the stacked final 3x3 convs, the protonet's `_output_layer`): the fp32
                accumulator is stored, no u |ref| term. The stacked conv has zero weight rows and zero
                bias up to a multiple of 4 columns (planner_yolact_head.cpp final_conv): the graph
                carries them, so the padding columns must come out as exact zeros.
              fp32: pack_op_host stores the fp32 weights it folded, the operands are exact: r_seg = 0 and
              the bound is K 2^-24 A + 2^-24 |ref|.
 stage        the ResNet input staging (aux.hip prep_nchw): pixel (y, x) holds the 7 x 3 values
              img[c, y, x + kx - 3] (zero outside the row) at channel 3 kx + c, zeros in channels
              21..23; one rounding of the fp32 pixel: u |ref| (fp32: exact). The stem is then the
              engine's own GEMM: 7 x 1 taps over 24 channels at stride 2, pad (3, 0).
 layout_in    aux.hip nchw_to_nhwc: one rounding of the fp32 input, u |ref| (fp32: exact).
 maxpool      resnet.hip maxpool3x3s2: the max of stored values, converted back to the dtype they had:
              exact, bound 0. Behind the fused stem7s2_pool neither the staged image nor the conv is
              stored: see "unstored tensors".
 add_relu     resnet.hip add_relu: `(T)fmaxf((float)a + (float)b, 0)`: one fp32 add (2^-24 (|a| + |b|))
              and one rounding (u |ref|); Q = 0.
 store_f32    resnet.hip store_f32: a widening conversion, exact: bound 0.
 bilinear_add yolact_head.hip bilinear_add against F.interpolate(mode="bilinear",
              align_corners=False) + add in float64. The kernel blends the four stored taps in fp32
              (3 fma + 2 mul, each within 2^-24 of a partial sum <= U = the tap-weighted |source|),
              rounds the interpolated value to T (u U), adds the stored lateral in fp32 and rounds the
              sum (u |ref|). Its tap weights come from fp32 index arithmetic: `scale = in / out`
              rounded, one fma: the source coordinate is within 2^-23 (in + 1) of the exact one, so
              each of the two 1-D weights is, and the blend moves by at most that, per axis, times the
              four |taps| <= 4 max|source| of the frame's channel. With A = U + |lateral|:
                det = u U (1 + u) + u |ref| + 8 2^-24 A + 2^-23 (hs + ws + 2) 4 max|source|
                stat scale = u (|ref| + U)   (the one rounding the reference does not have)
 convt3       ConvTranspose2d(3, 2, 1, output_padding=1) + LeakyReLU (convt3.hip, or the four phase
              GEMMs of planner_protonet.cpp): output (2m + pi, 2n + pj) sums (1 + pi)(1 + pj) taps x
              cin channels, so K is per output phase cin, 2 cin, 2 cin or 4 cin; weights rounded
              (r = 1), fp32 accumulation, LeakyReLU 1-Lipschitz, one output rounding.
              A = conv_transpose(|x|, |w|) + |bias|. The engine has four ops (one per phase) that share
              one output tensor: the graph has the whole ConvTranspose under the phase-(0,0) label and
              three "phase" rows that are reported as not stored; where the phases run as GEMMs of
              their own (TV_CT3=0, fp32) every op's snapshot is that shared tensor and only the last
              one is complete: check() judges that one.
 head_scatter yolact_head.hip head_scatter, from the stored fp32 raw tensor of the level: the
              classification and box columns are a copy to row off_l + (y W + x) n_ar + a (bound 0),
              the mask coefficients `tanhf` of it. No accuracy statement for the device tanhf was found
              in the documentation installed with ROCm, so the project's fp32 bar holds: 1e-4
              absolute (tanh's scale is 1) against float64 tanh of the stored raw value; the measured
              maximum is recorded (LayerReport.tanh_err).

Unstored tensors (P). A tensor that an op computes but does not store (the fused stem7s2_pool's staged
image and conv1 output, the protonet's `_layers_3` when `_output_layer` runs in its epilogue) cannot
be teacher-forced: the float64 value passes through, and its own bound (det, stat) is propagated into
the next stored op instead of layer_ref's counter r = 1 + (rounded tensors behind the segment):
through a conv segment as conv(det, |w|) (added to det) and conv(stat^2, w^2) (added under the root
of the statistical scale), through the max-pool as the window maximum — ReLU, LeakyReLU and max are
1-Lipschitz. For the stem this is the window maximum of the conv bound with r = 2 (staged image and
weights: conv(u |x|, |w|) = u A), as tests/test_gpu_resnet18_stem.py derives it. The protonet's
unstored `_layers_3` is not rounded: conv3x3 EPI 1 feeds the 1x1 the fp32 activation as a hi + lo pair
(u^2 |v| left), so its propagated bound has no u |ref| term.

The statistical constant. c is measured on the CPU over every layer of every GPU case of
tests/test_gpu_yolact_layers.py in the reference arithmetic (emulate()), kept apart from layer_ref's
(C_MEASURED_YOLACT), and asserted on the GPU at twice that. fp32 is judged by the deterministic bound
alone: with exact operands the error is all fp32 accumulation, which grows like sqrt(K) 2^-24 Q in an
order-dependent way that u (|ref| + Q) does not describe; its statistical ratio is recorded only.
"""
import numpy as np
import torch
import torch.nn.functional as F

import layer_ref as LR
from layer_ref import Layer, LayerReport, ratios

IMG = LR.IMG
STAGE = "input staging (NCHW fp32 -> NHWC)"
BB = "_backbone._feature_extractor."
FP, MN, PH = "_feature_pyramid.", "_masknet.", "_prediction_head."
U = LR.U
# Largest err / (u (|ref| + Q)) of the emulated reference arithmetic over every layer of every GPU case
# (test_yolact_layer_ref_cpu.test_emulation_within_bounds_and_measures_c), and the asserted constant
C_MEASURED_YOLACT = {"fp16": 1.92, "bf16": 2.03}
C_STAT_YOLACT = {p: 2.0 * v for p, v in C_MEASURED_YOLACT.items()}
TANH_BAR = 1e-4  # absolute, on tanh's (-1, 1)
# half the smallest subnormal of the dtype: a rounding is within max(u |x|, ETA) of x
ETA = {"fp16": 2.0 ** -25, "bf16": 2.0 ** -134, "fp32": 2.0 ** -150}


class Op(Layer):
    """An engine op that is no conv: kind, the labels it reads (srcs), and the kind's own fields."""

    def __init__(self, label, kind, srcs, **fields):
        super().__init__(label, kind, [], None)
        self.srcs = list(srcs)
        self.__dict__.update(fields)

    def sources(self):
        return list(self.srcs)


def _conv(label, segs, bias, act, exact=(), out_f32=False, K=None):
    layer = Layer(label, "conv", segs, bias, act, None, out_f32, K)
    layer.exact = set(exact)   # sources whose segment has exact weights (the plain identity)
    layer.hi_lo = False        # if not stored: carried at ~fp32 (conv3x3 EPI 1), not rounded
    return layer


def _fold(sd, conv, bn=None):
    """Engine::fold in float64: (folded weight, shift) of a conv (its bias optional) + eval BatchNorm."""
    w = sd[conv + ".weight"].double()
    b = sd[conv + ".bias"].double() if conv + ".bias" in sd else torch.zeros(w.shape[0], dtype=torch.float64)
    if bn is None:
        return w, b
    s, t = _bn(sd, bn)
    return w * s.view(-1, 1, 1, 1), b * s + t


def _bn(sd, bn):
    """(scale, shift) of an eval BatchNorm."""
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
    return s, sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s


def _eye(c, scale=None):
    w = torch.eye(c, dtype=torch.float64)
    if scale is not None:
        w = w * scale.view(-1, 1)
    return w.view(c, c, 1, 1)


def _adder(layers):
    def add(layer):
        assert layer.label not in layers, layer.label
        layers[layer.label] = layer
        return layer.label
    return add


# ---- the graphs ----

def resnet18_layers(sd, pre="", store=True, layers=None):
    """append_resnet18 (+ build_plan_resnet's staging and, for TV_ARCH_RESNET18, fp32 stores):
    ({label: Layer} in plan order, the three taps' labels)."""
    layers = {} if layers is None else layers
    add = _adder(layers)
    add(Op(STAGE, "stage", [IMG]))
    w7, b = _fold(sd, pre + "conv1", pre + "bn1")
    we = torch.zeros((64, 24, 7, 1), dtype=torch.float64)  # K index = ky * 24 + kx * 3 + c (row-expanded)
    we[:, :21, :, 0] = w7.permute(0, 3, 1, 2).reshape(64, 21, 7)
    x = add(_conv(pre + "conv1 + bn1 + ReLU", [(STAGE, we, 2, (3, 0))], b, 1, K=147))
    x = add(Op(pre + "maxpool", "maxpool", [x]))
    taps = []
    for L in range(1, 5):
        c = 64 << (L - 1)
        for blk in range(2):
            p = f"{pre}layer{L}.{blk}"
            stride = 2 if (blk == 0 and L > 1) else 1
            w1, b1 = _fold(sd, p + ".conv1", p + ".bn1")
            h = add(_conv(p + ".conv1 + bn1 + ReLU", [(x, w1, stride, 1)], b1, 1))
            w2, b2 = _fold(sd, p + ".conv2", p + ".bn2")
            if blk and L > 1:
                tap = add(_conv(p + ".conv2 + bn2 (tap)", [(h, w2, 1, 1)], b2, 0))
                taps.append(tap)
                if L < 4:
                    x = add(Op(p + " relu(bn2 + x)", "add_relu", [tap, x]))
            elif stride == 2:
                wd, bd = _fold(sd, p + ".downsample.0", p + ".downsample.1")
                x = add(_conv(p + ".conv2 + bn2 + downsample + ReLU", [(h, w2, 1, 1), (x, wd, 2, 0)], b2 + bd, 1))
            else:
                x = add(_conv(p + ".conv2 + bn2 + x + ReLU", [(h, w2, 1, 1), (x, _eye(c), 1, 0)], b2, 1, exact=[x]))
    if store:
        for i, t in enumerate(taps):
            add(Op(f"layer{i + 2}.1.bn2 -> fp32 NHWC", "store_f32", [t]))
    return layers, taps


def protonet_layers(sd, pre, x, layers):
    """append_protonet on the tensor of label x."""
    add = _adder(layers)

    def conv3(name, src):
        w, b = _fold(sd, pre + name)
        return add(_conv(pre + name + " + LeakyReLU", [(src, w, 1, 1)], b, 2))

    def up(name, src):
        labels = [f"{pre}{name} phase ({ph >> 1},{ph & 1}) + LeakyReLU" for ph in range(4)]
        add(Op(labels[0], "convt3", [src], w=sd[pre + name + ".weight"].double(),
               bias=sd[pre + name + ".bias"].double(), phases=labels))
        for lb in labels[1:]:
            add(Op(lb, "phase", [], of=labels[0]))
        return labels[0]

    x = conv3("_layers_1.0.0", x)
    x = up("_upsample_layer_1", x)
    x = conv3("_layers_2.0.0", x)
    x = up("_upsample_layer_2", x)
    x = conv3("_layers_3.0.0", x)
    layers[x].hi_lo = True
    w, b = _fold(sd, pre + "_output_layer")
    k = w.shape[0]
    kp = (k + 3) // 4 * 4
    wp = torch.zeros((kp,) + tuple(w.shape[1:]), dtype=torch.float64)
    bp = torch.zeros(kp, dtype=torch.float64)
    wp[:k], bp[:k] = w, b
    return add(_conv(pre + "_output_layer + LeakyReLU -> fp32 NHWC", [(x, wp, 1, 0)], bp, 2, out_f32=True))


def yolact_head_layers(sd, n_levels, down, heights, n_ar, taps=None, layers=None):
    """append_yolact_head (the head archs): ({label: Layer} in plan order, the FPN levels' labels, the
    prototypes' label). taps: the backbone maps' labels when they are tensors of the plan already
    (TV_ARCH_YOLACT); otherwise input i is read from the source "map<i>" through a layout op."""
    layers = {} if layers is None else layers
    add = _adder(layers)
    Fd = sd[FP + "_lateral_layers.0.weight"].shape[0]
    lat = []
    for i in range(n_levels):
        x = taps[i] if taps else add(Op(f"backbone map {i} NCHW fp32 -> NHWC", "layout_in", [f"map{i}"]))
        name = f"{FP}_lateral_layers.{i}"
        w, b = _fold(sd, name)
        lat.append(add(_conv(name, [(x, w, 1, 0)], b, 0)))
    pyr = list(lat)
    for i in range(n_levels - 2, -1, -1):  # in place on the lateral's tensor: later readers see the sum
        pyr[i] = add(Op(f"pyramid {i} = lateral + bilinear(pyramid {i + 1})", "bilinear_add", [pyr[i + 1], lat[i]]))
    lv = []
    for i in range(n_levels):
        name = f"{FP}_prediction_layers.{i}"
        w, b = _fold(sd, name)
        lv.append(add(_conv(name + " + LeakyReLU", [(pyr[i], w, 1, 1)], b, 2)))
    for i in range(down):
        name = f"{FP}_downsample_layers.{i}"
        w, b = _fold(sd, name)
        lv.append(add(_conv(name + " + LeakyReLU", [(lv[-1], w, 2, 1)], b, 2)))
    proto = protonet_layers(sd, MN, lv[0], layers)

    def blocks(lp, g, n, x):
        for i in range(n):
            bk = f"{PH}{g}_layers.{i}"
            w, b = _fold(sd, bk + ".conv1", bk + ".bn1")
            t1 = add(_conv(lp + bk + ".conv1", [(x, w, 1, 0)], b, 1))
            w, b = _fold(sd, bk + ".conv2", bk + ".bn2")
            t2 = add(_conv(lp + bk + ".conv2", [(t1, w, 1, 1)], b, 1))
            w, b = _fold(sd, bk + ".conv3", bk + ".bn3")
            y = add(_conv(lp + bk + ".conv3 + x", [(t2, w, 1, 0), (x, _eye(Fd), 1, 0)], b, 1, exact=[x]))
            cv = f"{PH}{g}_conv_layers.{i}"
            w, b = _fold(sd, cv)
            s, t = _bn(sd, f"{PH}{g}_bn_layers.{i}")
            x = add(_conv(f"{lp}{cv} + {g}_bn_layers.{i}(bottleneck)", [(x, w, 1, 0), (y, _eye(Fd, s), 1, 0)],
                          b + t, 1))
        return x

    def final(label, x, names):
        ws, bs = zip(*[_fold(sd, n) for n in names])
        w, b = torch.cat(ws, 0), torch.cat(bs, 0)
        n = w.shape[0]
        npad = (n + 3) // 4 * 4  # the fp32 store writes whole 16-byte vectors: zero weight rows up to it
        wp = torch.zeros((npad,) + tuple(w.shape[1:]), dtype=torch.float64)
        bp = torch.zeros(npad, dtype=torch.float64)
        wp[:n], bp[:n] = w, b
        return add(_conv(label, [(x, wp, 1, 1)], bp, 0, out_f32=True)), [v.shape[0] for v in ws]

    fin = [PH + "_classification_layer", PH + "_box_encoding_layer", PH + "_mask_coeff_layer"]
    stacked = not heights[1] and not heights[2] and not heights[3]
    for l, f in enumerate(lv):
        lp = f"level {l} "
        x = blocks(lp, "_extra", heights[0], f)
        parts = []  # (raw label, first column, columns, is the mask coefficients)
        if stacked:
            raw, ns = final(lp + "final 3x3 convs (stacked)", x, fin)
            c0 = 0
            for j, n in enumerate(ns):
                parts.append((raw, c0, n, j == 2))
                c0 += n
        else:
            for j, g in enumerate(("_classification_extra", "_box_extra", "_mask_extra")):
                raw, ns = final(lp + fin[j], blocks(lp, g, heights[1 + j], x), [fin[j]])
                parts.append((raw, 0, ns[0], j == 2))
        add(Op(lp + "raw heads -> classification / box_encoding / tanh(mask_coeff)", "head_scatter",
               [p[0] for p in parts], parts=parts, n_ar=n_ar))
    return layers, lv, proto


def yolact_layers(sd, down, heights, n_ar):
    """build_plan_resnet for TV_ARCH_YOLACT: the backbone under `_backbone._feature_extractor.`, its
    taps feeding the lateral convs from the arena (no fp32 store, no layout op)."""
    layers, taps = resnet18_layers(sd, BB, store=False)
    return yolact_head_layers(sd, 3, down, heights, n_ar, taps=taps, layers=layers)


# ---- one layer ----

def _expand(img):
    """prep_nchw's row-expanded staging of an NCHW image: [B, 24, H, W]."""
    B, _, H, W = img.shape
    p = F.pad(img, (3, 3))
    out = torch.zeros((B, 24, H, W), dtype=img.dtype)
    for kx in range(7):
        out[:, 3 * kx:3 * kx + 3] = p[..., kx:kx + W]
    return out


def _scatter_rows(r, n_ar):
    """[B, n_ar * width, H, W] -> [B, H W n_ar, width], row (y W + x) n_ar + a, column j = channel a width + j."""
    B, n, H, W = r.shape
    return r.reshape(B, n_ar, n // n_ar, H, W).permute(0, 3, 4, 1, 2).reshape(B, H * W * n_ar, n // n_ar)


def _convt3(x, w, b):
    return F.leaky_relu(F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1), 0.01)


def evaluate(layer, xs):
    """The layer in the dtype of its inputs (float64: the reference). head_scatter: the level's
    (classification, box, mask coefficient) row blocks."""
    k = layer.kind
    if k == "conv":
        return LR.evaluate(layer, xs)
    x = xs[layer.srcs[0]]
    if k == "stage":
        return _expand(x)
    if k in ("layout_in", "store_f32"):
        return x
    if k == "maxpool":
        return F.max_pool2d(x, 3, 2, 1)
    if k == "add_relu":
        return F.relu(x + xs[layer.srcs[1]])
    if k == "bilinear_add":
        lat = xs[layer.srcs[1]]
        return lat + F.interpolate(x, lat.shape[2:], mode="bilinear", align_corners=False)
    if k == "convt3":
        return _convt3(x, layer.w.to(x.dtype), layer.bias.to(x.dtype))
    if k == "head_scatter":
        out = []
        for raw, c0, n, is_coef in layer.parts:
            r = _scatter_rows(xs[raw][:, c0:c0 + n], layer.n_ar)
            out.append(torch.tanh(r) if is_coef else r)
        return tuple(out)
    raise ValueError(k)


def emulate(layer, xs, precision):
    """The reference arithmetic of a correct kernel (module docstring, per kind), float64 result."""
    dt = LR.TORCH_DTYPE[precision]
    k = layer.kind

    def q(t):
        return t.to(dt).double()
    if k == "conv":
        return LR.emulate(layer, xs, precision)
    if k in ("maxpool", "store_f32"):
        return evaluate(layer, xs)
    x = xs[layer.srcs[0]].float()
    if k == "stage":
        return q(_expand(x))
    if k == "layout_in":
        return q(x)
    if k == "add_relu":
        return q(F.relu(x + xs[layer.srcs[1]].float()))
    if k == "bilinear_add":
        lat = xs[layer.srcs[1]].float()
        up = F.interpolate(x, lat.shape[2:], mode="bilinear", align_corners=False).to(dt).float()
        return q(lat + up)
    if k == "convt3":
        return q(_convt3(x, layer.w.float().to(dt).float(), layer.bias.float()))
    if k == "head_scatter":
        out = []
        for raw, c0, n, is_coef in layer.parts:
            r = _scatter_rows(xs[raw][:, c0:c0 + n].float(), layer.n_ar)
            out.append((torch.tanh(r) if is_coef else r).double())
        return tuple(out)
    raise ValueError(k)


def _f32(layer):
    """The conv layer with float32 weights, for the bound scales A and Q (made once)."""
    if not hasattr(layer, "_w32"):
        layer._w32 = [w.float() for _, w, _, _ in layer.segs]
    return layer._w32


def lin_index(n_out, n_in):
    """torch's bilinear source index (align_corners=False) in float64: (i0, i1, l0, l1) per output index."""
    d = torch.arange(n_out, dtype=torch.float64)
    src = ((n_in / n_out) * (d + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    l1 = (src - i0).clamp(0.0, 1.0)
    return i0, i1, 1.0 - l1, l1


def bilinear(x, size, clamp=True):
    """F.interpolate(x, size, mode="bilinear") by gathers. clamp=False: the second tap's index is not
    clamped to the last row / column (a fault the tests inject): it reads the next row's first pixel,
    or, past the last row, zero."""
    H, W = x.shape[2:]
    h0, h1, a0, a1 = lin_index(size[0], H)
    w0, w1, b0, b1 = lin_index(size[1], W)
    if not clamp:  # i1 = i0 + 1 on a flat [H * W (+ one zero row)] frame
        flat = F.pad(x, (0, 0, 0, 2)).reshape(x.shape[0], x.shape[1], -1)

        def at(r, c):
            return flat[:, :, (r.view(-1, 1) * W + c.view(1, -1))]
        h1, w1 = h0 + 1, w0 + 1
        top = at(h0, w0) * b0 + at(h0, w1) * b1
        bot = at(h1, w0) * b0 + at(h1, w1) * b1
    else:
        rows0, rows1 = x[:, :, h0], x[:, :, h1]
        top = rows0[..., w0] * b0 + rows0[..., w1] * b1
        bot = rows1[..., w0] * b0 + rows1[..., w1] * b1
    return top * a0.view(-1, 1) + bot * a1.view(-1, 1)


def bounds(layer, xs, ref, precision, pend=None):
    """(deterministic bound, statistical scale) per element; pend = {source label: (det, stat) of an
    unstored source}, propagated as the module docstring says. Scales in float32, returned as float64."""
    pend = pend or {}
    u = U[precision]
    uw = 0.0 if precision == "fp32" else u   # rounding of an operand to the compute dtype (fp32: exact)
    eta = ETA[precision]
    k = layer.kind
    aref = ref.abs() if torch.is_tensor(ref) else None
    if k == "conv":
        A = Aw = Q2 = P = S2 = 0.0
        for (src, _, stride, pad), w in zip(layer.segs, _f32(layer)):
            x = xs[src].float()
            a = F.conv2d(x.abs(), w.abs(), None, stride, pad)
            A = A + a
            if src not in layer.exact:
                Aw = Aw + a
                Q2 = Q2 + F.conv2d(x * x, w * w, None, stride, pad)
            if src in pend:
                pd, ps = pend[src]
                P = P + F.conv2d(pd.float(), w.abs(), None, stride, pad)
                S2 = S2 + F.conv2d((ps * ps).float(), w * w, None, stride, pad)
        det = uw * Aw + layer.K * 2.0 ** -24 * A + P
        stat = torch.sqrt(u * u * Q2 + S2)
        det, stat = torch.as_tensor(det).double(), torch.as_tensor(stat).double()
        if not layer.out_f32:
            det = det + u * aref + eta
        return det, stat + u * aref + eta
    assert k == "maxpool" or not any(s in pend for s in layer.sources()), (layer.label, "reads an unstored tensor")
    if k in ("stage", "layout_in"):
        return (uw * aref + eta, uw * aref + eta) if uw else (uw * aref, uw * aref)
    if k == "store_f32":
        return torch.zeros_like(ref), torch.zeros_like(ref)
    if k == "maxpool":
        src = layer.srcs[0]
        if src in pend:
            return F.max_pool2d(pend[src][0], 3, 2, 1), F.max_pool2d(pend[src][1], 3, 2, 1)
        return torch.zeros_like(ref), torch.zeros_like(ref)
    if k == "add_relu":
        A = xs[layer.srcs[0]].abs() + xs[layer.srcs[1]].abs()
        return u * aref + eta + 2.0 ** -24 * A, u * aref + eta
    if k == "bilinear_add":
        x, lat = xs[layer.srcs[0]], xs[layer.srcs[1]]
        Uup = bilinear(x.abs(), lat.shape[2:])
        A = Uup + lat.abs()
        wgt = 2.0 ** -23 * (x.shape[2] + x.shape[3] + 2) * 4.0 * x.abs().amax((2, 3), keepdim=True)
        return uw * Uup * (1 + u) + u * aref + 2 * eta + 8 * 2.0 ** -24 * A + wgt, u * (aref + Uup) + 2 * eta
    if k == "convt3":
        x, w = xs[layer.srcs[0]].float(), layer.w.float()
        kw = dict(stride=2, padding=1, output_padding=1)
        A = F.conv_transpose2d(x.abs(), w.abs(), layer.bias.float().abs(), **kw).double()
        Q = torch.sqrt(F.conv_transpose2d(x * x, w * w, None, **kw)).double()
        par = torch.arange(ref.shape[2]) % 2, torch.arange(ref.shape[3]) % 2
        K = w.shape[0] * (1 + par[0]).view(-1, 1) * (1 + par[1]).view(1, -1)  # cin x taps of the output phase
        return uw * A + K.double() * 2.0 ** -24 * A + u * aref + eta, u * (aref + Q) + eta
    raise ValueError(k)


def pending(layer, ref, det, stat, precision):
    """The (det, stat) an unstored layer hands to its readers."""
    if layer.kind == "conv" and layer.hi_lo and not layer.out_f32:  # carried as hi + lo: u^2 |v| instead of u |v|
        u = U[precision]
        return det - u * ref.abs() - ETA[precision] + u * u * ref.abs(), stat - u * ref.abs() - ETA[precision]
    return det, stat


def _tile(kernel, idx, layer, xs):
    if layer.kind == "conv" and all(isinstance(p, int) for _, _, _, p in layer.segs):
        return LR.tile_of(kernel, idx, layer, xs)
    b, _, y, x = idx
    return f"pixel ({y}, {x}) of frame {b}"


def check(layers, inputs, precision, stored, kernels=None, heads=None):
    """Teacher-forced per-layer comparison. layers: a graph above; inputs: {IMG: float64 NCHW image} or
    {"map<i>": float64 NCHW map}; stored: {label: float64 NCHW tensor the engine stored for that op, or
    None}; heads: the caller's (classification, box_encoding, mask_coeff) float64 [B, A, width], which
    the head_scatter ops wrote. Returns a LayerReport with one row per judged layer (c for
    LayerReport.failures: C_STAT_YOLACT)."""
    missing = [k for k in layers if k not in stored]
    extra = [k for k in stored if k not in layers]
    assert not missing and not extra, f"no engine op with the labels {missing}; no layer for the engine's ops {extra}"
    kernels = kernels or {}
    vals, pend, depth = dict(inputs), {}, {k: 0 for k in inputs}
    rep = LayerReport()
    rep.tanh_err = 0.0
    row = 0
    for label, layer in layers.items():
        if layer.kind == "phase":  # its pixels are judged with the whole ConvTranspose, at the phase-(0,0) row
            rep.skipped.append(label)
            continue
        xs = {s: vals[s] for s in layer.sources()}
        ref = evaluate(layer, xs)
        r = 1 + max(depth[s] for s in layer.sources())
        kern = kernels.get(label, "")
        if layer.kind == "head_scatter":
            assert stored[label] is None and heads is not None
            n = ref[0].shape[1]
            worst, at = 0.0, (0, 0, 0, 0)
            for j, (want, (_, _, _, is_coef)) in enumerate(zip(ref, layer.parts)):
                got = heads[j][:, row:row + n]
                assert got.shape == want.shape, (label, j, tuple(got.shape), tuple(want.shape))
                err = (got - want).abs()
                if is_coef:
                    rep.tanh_err = max(rep.tanh_err, float(err.max()))
                    rd = err / TANH_BAR
                else:
                    rd = torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf")))
                if float(rd.max()) >= worst:
                    worst = float(rd.max())
                    b, a, c = (int(v) for v in np.unravel_index(int(torch.argmax(rd)), tuple(rd.shape)))
                    at = (b, c, row + a, j)
            rep.rows.append((label, kern, r, worst, worst, at,
                             f"output {at[3]}, anchor row {at[2]} (y = row, x = output)"))
            row += n
            continue
        got = stored[label]
        if layer.kind == "convt3" and stored[layer.phases[-1]] is not None:
            got = stored[layer.phases[-1]]  # phase GEMMs of their own: the snapshot after the last one is complete
        det, stat = bounds(layer, xs, ref, precision, pend)
        if got is None:
            pend[label] = pending(layer, ref, det, stat, precision)
            vals[label] = ref
            depth[label] = r - 1 + (0 if getattr(layer, "hi_lo", False) else 1)
            rep.skipped.append(label)
            continue
        assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
        rd, rs = ratios(got, ref, det, stat)
        idx = tuple(int(v) for v in np.unravel_index(int(torch.argmax(rd)), tuple(rd.shape)))
        rep.rows.append((label, kern, r, float(rd.max()), float(rs.max()), idx, _tile(kern, idx, layer, xs)))
        vals[label], depth[label] = got, 0
    assert len(rep.rows) + len(rep.skipped) == len(layers)
    assert heads is None or row == heads[0].shape[1], (row, tuple(heads[0].shape))
    return rep


def forward(layers, inputs, step):
    """Every layer by step(layer, xs), without forcing: ({label: tensor}, the three head outputs or None)."""
    vals = dict(inputs)
    blocks = []
    for label, layer in layers.items():
        if layer.kind == "phase":
            continue
        out = step(layer, {s: vals[s] for s in layer.sources()})
        if layer.kind == "head_scatter":
            blocks.append(out)
        else:
            vals[label] = out
    heads = tuple(torch.cat([b[j] for b in blocks], 1) for j in range(3)) if blocks else None
    return vals, heads


def forward64(layers, inputs):
    return forward(layers, inputs, evaluate)


def emulated_forward(layers, inputs, precision):
    """The whole forward in the reference arithmetic (the CPU stand-in for the engine's stored tensors):
    ({label: float64 tensor or None}, heads), every tensor stored, the phase rows None."""
    vals, heads = forward(layers, {k: v.float().double() for k, v in inputs.items()},
                          lambda layer, xs: emulate(layer, xs, precision))
    return {k: vals.get(k) for k in layers}, heads


# ---- the cases of tests/test_gpu_yolact_layers.py ----

# image (h, w, B): module docstring of tests/test_gpu_yolact_layers.py
BACKBONE_GEOMETRIES = {"R1": (200, 280, 3), "R2": (149, 77, 1), "R3": (37, 51, 5)}
_HEAD = dict(depths=(128, 256, 512), C=7, k=8, layers=(1, 0, 0, 0), down=2)
HEAD_GEOMETRIES = {
    "H1": dict(_HEAD, name="H1", F=256, ars=(1, 2), sizes=((13, 18), (7, 9), (4, 5)), batch=3, seed=610),
    "H2": dict(_HEAD, name="H2", F=256, ars=(1,), sizes=((25, 35), (13, 18), (7, 9)), batch=1, seed=620),
    "H3": dict(_HEAD, name="H3", F=128, ars=(1,), sizes=((13, 18), (7, 9), (4, 5)), batch=3, seed=630),
}
# the whole model: R2's image (taps 19x10, 10x5, 5x3), H1's head fields, B = 2
WHOLE = dict(_HEAD, name="W", F=256, ars=(1, 2), in_h=149, in_w=77, batch=2, seed=640)
for _c in HEAD_GEOMETRIES.values():
    _c["in_h"], _c["in_w"] = 8 * _c["sizes"][0][0], 8 * _c["sizes"][0][1]


def f64(sd):
    return {k: v.double() for k, v in sd.items() if v.dtype.is_floating_point}


def backbone_case(name, B=None):
    """(seeded state dict as loaded, its float64 copy, fp32 NCHW image) of a backbone geometry."""
    import resnet18_ref as rr
    h, w, b0 = BACKBONE_GEOMETRIES[name]
    sd = rr.seeded_resnet18_state_dict(seed=31)
    img = torch.randn((B or b0, 3, h, w), generator=torch.Generator().manual_seed(h * 1000 + w))
    return sd, f64(sd), img


def head_config(c):
    from recipe_yolact_head import SCALES, VAR
    from tauv_vision_amd.yolact import YolactConfig
    return YolactConfig(c["in_w"], c["in_h"], SCALES, c["ars"], VAR, c["F"], c["k"], c["C"], *c["layers"], c["down"])


def head_case(name):
    """(case, seeded state dict, its float64 copy, fp32 NCHW maps) of a head geometry."""
    from recipe_yolact_head import head_inputs
    from tauv_vision_amd.weights import param_layout, yolact_head_desc
    c = HEAD_GEOMETRIES[name]
    layout = param_layout(yolact_head_desc(c["depths"], c["sizes"], c["F"], c["down"], c["C"], c["k"], len(c["ars"]),
                                           c["layers"]))
    sd, maps = head_inputs(c, layout=layout)
    return c, sd, f64(sd), maps


def whole_case():
    """(case, seeded whole-model state dict, its float64 copy, fp32 NCHW image)."""
    import resnet18_ref as rr
    from recipe_yolact_head import head_inputs
    from tauv_vision_amd.weights import param_layout, yolact_desc
    c = WHOLE
    layout = [(k, s) for k, s in param_layout(yolact_desc(c["in_h"], c["in_w"], c["F"], c["down"], c["C"], c["k"],
                                                          len(c["ars"]), c["layers"])) if not k.startswith(BB)]
    head_sd, _ = head_inputs(dict(c, sizes=(), depths=()), layout=layout)
    sd = {BB + k: v for k, v in rr.seeded_resnet18_state_dict(seed=32).items()}
    sd.update(head_sd)
    img = torch.randn((c["batch"], 3, c["in_h"], c["in_w"]), generator=torch.Generator().manual_seed(c["seed"] + 5))
    return c, sd, f64(sd), img
