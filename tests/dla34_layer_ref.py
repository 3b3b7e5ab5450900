"""Per-layer reference for the native CenterpointDLA34 plan (TV_ARCH_DLA34, csrc/planner_dla34.cpp): the
method of tests/layer_ref.py and tests/yolact_layer_ref.py — every engine op judged on its own, from the
tensors the engine stored (teacher forcing), under a derived deterministic bound and a CPU-measured
statistical one — applied to the ops only this plan has.

dla34_layers() restates the planner's forward lowering from a reference-layout state dict (keys `model.*`):
one Layer per engine op, in plan order, under the engine's labels (tv_engine_op_label). The plan labels
every pooling op "MaxPool2d(2, 2, ceil_mode=True)": unique_labels() numbers repeated labels in plan order,
for the graph and for the engine's list alike. check() refuses a label the engine has and the graph
lacks, or the reverse. tests/test_dla34_layer_ref_cpu.py shows that the graph, evaluated in float64
without forcing, is oracle.ref_dla34.dlaseg_forward to 1e-9.

Notation as yolact_layer_ref: u the unit roundoff of the compute dtype (2^-11 fp16, 2^-8 bf16, 2^-24
fp32), ETA half its smallest subnormal, A = sum |x_k| |w_k|, Q = sqrt(sum x_k^2 w_k^2), K the reduction
length, per output element

  deterministic   |got - ref| <= u sum_seg r_seg A_seg + K 2^-24 A + u |ref| + ETA      (+ P, S below)
  statistical     |got - ref| <= c (u (|ref| + Q) + ETA)

Layer kinds and where their bounds come from:

 conv         yolact_layer_ref's conv (bounds() there), for
              * the row-expanded 7x7 stem over the staged image (7 x 1 taps over 24 channels, K = 147,
                pad (3, 0)) and the level0 / level1 convs (C = 16, 32);
              * BasicBlock `conv2+residual`: the residual is a second K-segment, Tree.project's 1x1 + BN
                folded over the max-pooled bottom (r_seg = 1), or an identity segment whose stored
                weight is exactly 1 (pack_op_host `sg.identity`: r_seg = 0, nothing in Q);
              * the Root 1x1 over torch.cat(children): one K-segment per child in the reference's order
                (x2, x1, *children), segment j reading input channels [ci0_j, ci0_j + C_j) of the one
                `root.conv.weight` (level 3: 128 + 128 + 64 + 128, level 5: 512 + 512 + 256);
              * the offset + mask conv: the 18-row `offset` and 9-row `mask` 3x3 weights stacked, padded
                to 32 rows with zero weights and zero bias, no activation (planner_dla34.cpp deform():
                `om.N = 32`). Columns 27..31 must be exact zeros: check() asserts it beside the bound;
              * the stacked 3x3 heads (N = 256 x heads, bias, ReLU) and the block-diagonal 1x1 heads into
                the fp32 output (out_f32: no u |ref| term; K = 256; zero rows up to a multiple of 4).
              fp32: operands exact, r_seg = 0.
 stage        OP_PREP: pixel (y, x) holds the 7 x 3 values img[c, y, x + kx - 3] at channel 3 kx + c,
              zeros in 21..23; one rounding of the fp32 pixel or u8 LUT entry (u |ref| + ETA). Where
              stem.hip absorbs it (`prep (fused into the stem)`) nothing is stored and the bound
              propagates into the stem (yolact_layer_ref "unstored tensors": conv(u |x|, |w|) = u A).
 maxpool      dla34.hip maxpool2_ceil against F.max_pool2d(x, 2, 2, ceil_mode=True) of the stored
              tensor: fmaxf over values converted to fp32 and back to the dtype they had: exact, bound 0.
 dwconvt      dla34.hip dwconvt_add / dwconvt_add_p2 against F.conv_transpose2d(groups=C, stride=f,
              padding=f // 2) + ref_dla34.pad_to_match + skip in float64. The fp32 depthwise weight is
              read as it is, and the kernel sums in fp64 (`acc[e] += (double)t.v[e] * (double)wp[e]`,
              then `acc[e] + (double)s.v[e]`): every product is exact (at most 24 + 24 bits), the at most
              four adds and the add of the stored skip are each within 2^-53 of a partial sum <= A,
              A = sum |x| |w| + |skip|; the float64 reference sums the same terms with the same error,
              so e64 = 10 2^-53 A between the two. The sum is rounded to fp32 (`(float)(...)`, 2^-24) and
              then to T (store_vec, u; none for fp32 tensors):
                det = e64 + (2^-24 + u (1 + 2^-24)) (|ref| + e64) + ETA
              Q = 0: the statistical scale is u |ref| + ETA. (With an fp32 sum the kernel missed it
              wherever taps and skip nearly cancel: one element of tests/test_gpu_dla34_layers.py's
              halo / G1T / bf16 case, ref = -2.9e-9 where A = 2.4e-2, was at 6.43 x u |ref|.)
 dcn_sample / dcn
              The DCN op and its column GEMM, against oracle.ref_dla34.deform_conv2d in float64 from the
              stored x and the stored offset / mask tensor (sigmoid of the stored logits), the `actf`
              BatchNorm folded into weight and bias, ReLU. dcn_cols() below restates the sampling with
              its intermediate values (tests/test_dla34_layer_ref_cpu.py: its contraction is
              deform_conv2d to 1e-9). Per column element col[c, k] = m_k sum_corner wt_corner v_corner:
              * positions. dcn.hip / dla34.hip: `py = (float)(oy - 1 + k / 3) + dy`: the integer and the
                stored offset are exact in fp32, the sum is one rounding, so py and px are each within
                2^-24 |p| of the exact position; `ly = py - fy` is exact, `hy = 1 - ly` one rounding
                (counted below). The zero-padded bilinear sample is continuous in the position with
                slope at most the sum of the four |corner| values per axis (across a cell border and the
                -1 / H border too: the weights that change hands are zero there), so the displacement
                moves it by at most  D = 2 x 2^-23 (max(|py|, |px|) + 1) sum_corner |v|  (both axes; the
                issue's 2^-23 per axis covers the 2^-24 with room for the comparison done on the
                rounded position);
              * arithmetic. `hy`, `hy * hx`, `w4 * mask` (fused: the mask is folded into the corner
                weight; dcn_sample multiplies the sum instead: the same count) and four fmas: 7
                roundings, and 2 more in `1 / (1 + expf(-logit))` (add, divide): (1 + 2^-24)^9 - 1
                <= 9 2^-24 (1 + 2^-20) relative to m U, U = sum_corner wt |v|;
              * expf. No accuracy statement for the device expf was found in the documentation installed
                with ROCm (the same search that found none for tanhf, yolact_layer_ref head_scatter), so
                the project's existing treatment of a device transcendental holds: an absolute 1e-4 on
                the function's unit scale, here on sigmoid's (0, 1): SIG_BAR U per element. The fp32
                plan stores the columns: the ratios of its dcn_sample rows show how much of that the
                device uses.
                dcol = m U 9 2^-24 (1 + 2^-20) + SIG_BAR U + m D
              Unfused (fp32: dcn_sample, then the GEMM over the stored 9 C-channel column tensor, channel
              k C + c): two rows. dcn_sample: det = dcol (+ u |ref| + ETA where the columns are stored in
              a 16-bit dtype); the GEMM is a plain 1x1 conv over the stored columns (r = 0 in fp32).
              Fused (dcn.hip: DcnInFused / DcnFused): the OP_DCN row is reported as not stored and the
              GEMM row carries both. The sampled column is rounded to the compute dtype before the MFMA
              ("one rounding to T") and the weights are rounded (pack_op_host): r = 2 on A = sum |col| |w|,
              and the sampling error passes through the weights: S = sum |w| dcol. Split-K partials are
              fp32 sums of the same products (any order: the K 2^-24 term).
                det = (2 u (1 + u) + K 2^-24) (A + S) + S + u |ref| + ETA,   K = 9 C
                stat scale = u (|ref| + sqrt(2) Q) + S + ETA   (two independent roundings per product)

The statistical constant c is measured on the CPU over every layer of every GPU case of
tests/test_gpu_dla34_layers.py in the reference arithmetic (emulate()), kept apart from the other two
graphs' (C_MEASURED_DLA34) and asserted on the GPU at twice that. fp32 is judged by the deterministic
bound alone, as in yolact_layer_ref.
"""
import numpy as np
import torch
import torch.nn.functional as F

import layer_ref as LR
import yolact_layer_ref as YL
from layer_ref import LayerReport, ratios
from oracle import ref_dla34
from oracle.ref_dla34 import pad_to_match
from yolact_layer_ref import ETA, Op, _conv, _eye, _fold

IMG = LR.IMG
U = LR.U
STAGE = "input staging (NCHW fp32 / u8 frames -> NHWC)"
MAXPOOL = "MaxPool2d(2, 2, ceil_mode=True)"
HEADS_HIDDEN = "model.*.0 (stacked heads) + ReLU"
HEADS_OUT = "model.*.2 (block-diagonal) -> fp32 NHWC"
UP_F4 = "model.ida_up.up_2+pad_to_match+add"  # the only f = 4 step that shifts (7x.. -> 28x.. onto 25x..)
LEVELS = ref_dla34.DLA34_LEVELS
CHANNELS = ref_dla34.DLA34_CHANNELS
SIG_BAR = 1e-4  # absolute, on sigmoid's (0, 1): see the module docstring
# Largest err / (u (|ref| + Q) + ETA) of the emulated reference arithmetic over every layer of every GPU
# case (test_dla34_layer_ref_cpu.test_emulation_within_bounds_and_measures_c), and the asserted constant
C_MEASURED_DLA34 = {"fp16": 1.84, "bf16": 1.85}
C_STAT_DLA34 = {p: 2.0 * v for p, v in C_MEASURED_DLA34.items()}


def unique_labels(labels):
    """Plan-order labels with the k-th repeat (k >= 2) of a label renamed `label #k`."""
    seen, out = {}, []
    for lb in labels:
        seen[lb] = seen.get(lb, 0) + 1
        out.append(lb if seen[lb] == 1 else f"{lb} #{seen[lb]}")
    return out


# ---- the graph ----

def dla34_layers(sd):
    """build_plan_dla34's forward lowering: {label: Layer} in plan order."""
    layers, names = {}, []

    def add(layer):
        names.append(layer.label)
        layer.label = unique_labels(names)[-1]
        assert layer.label not in layers, layer.label
        layers[layer.label] = layer
        return layer.label

    pooled = {}

    def maxpool(x):
        if x not in pooled:
            pooled[x] = add(Op(MAXPOOL, "maxpool", [x]))
        return pooled[x]

    def conv_bn_relu(p_conv, p_bn, src, stride):
        w, b = _fold(sd, p_conv, p_bn)
        return add(_conv(p_conv, [(src, w, stride, 1)], b, 1))

    def basic(p, x, stride, res, res_bias, exact):
        t = conv_bn_relu(p + ".conv1", p + ".bn1", x, stride)
        w2, b2 = _fold(sd, p + ".conv2", p + ".bn2")
        return add(_conv(p + ".conv2+residual", [(t, w2, 1, 1), res], b2 + res_bias, 1, exact=exact))

    def root(p, kids):
        wf, b = _fold(sd, p + ".conv", p + ".bn")
        segs, off = [], 0
        for k in kids:
            c = width[k]
            segs.append((k, wf[:, off:off + c], 1, 0))
            off += c
        assert off == wf.shape[1], (p, off, tuple(wf.shape))
        layer = _conv(p + ".conv", segs, b, 1)
        layer.w_full = wf
        return add(layer)

    width = {}

    def tree(p, x, levels, stride, cin, cout, level_root, children):
        bottom = maxpool(x) if stride > 1 else x
        width[bottom] = cin
        children = list(children)
        if level_root:
            children.append(bottom)
        if levels == 1:
            if cin != cout:
                wr, br = _fold(sd, p + ".project.0", p + ".project.1")
                x1 = basic(p + ".tree1", x, stride, (bottom, wr, 1, 0), br, [])
            else:
                x1 = basic(p + ".tree1", x, stride, (bottom, _eye(cin), 1, 0), 0.0, [bottom])
            x2 = basic(p + ".tree2", x1, 1, (x1, _eye(cout), 1, 0), 0.0, [x1])
            width[x1] = width[x2] = cout
            out = root(p + ".root", [x2, x1] + children)
            width[out] = cout
            return out
        x1 = tree(p + ".tree1", x, levels - 1, stride, cin, cout, False, [])
        return tree(p + ".tree2", x1, levels - 1, 1, cout, cout, False, children + [x1])

    def deform(p, x, cho):
        wo, bo = _fold(sd, p + ".offset")
        wm, bm = _fold(sd, p + ".mask")
        w = torch.cat([wo, wm, torch.zeros((5,) + tuple(wo.shape[1:]), dtype=torch.float64)], 0)
        b = torch.cat([bo, bm, torch.zeros(5, dtype=torch.float64)], 0)
        om = _conv(p + ".offset+mask", [(x, w, 1, 1)], b, 0)
        om.zero_cols = 27
        om = add(om)
        col = add(Op(p + ".conv (DCNv2 sampling)", "dcn_sample", [x, om]))
        wf, bf = _fold(sd, p + ".conv", p + ".actf.0")
        assert wf.shape[0] == cho
        return add(Op(p + ".conv+actf", "dcn", [x, om], col=col, w=wf, bias=bf, K=9 * wf.shape[1]))

    def ida(p, ls, startp, endp, o):
        for i in range(startp + 1, endp):
            j = i - startp
            pr = deform(f"{p}.proj_{j}", ls[i], o)
            w = sd[f"{p}.up_{j}.weight"].double()
            up = add(Op(f"{p}.up_{j}+pad_to_match+add", "dwconvt", [pr, ls[i - 1]], w=w, f=w.shape[2] // 2))
            ls[i] = deform(f"{p}.node_{j}", up, o)

    add(Op(STAGE, "stage", [IMG]))
    b = "model.base"
    w7, sh = _fold(sd, b + ".base_layer.0", b + ".base_layer.1")
    we = torch.zeros((w7.shape[0], 24, 7, 1), dtype=torch.float64)  # K index = ky * 24 + kx * 3 + c (row-expanded)
    we[:, :21, :, 0] = w7.permute(0, 3, 1, 2).reshape(w7.shape[0], 21, 7)
    x = add(_conv(b + ".base_layer.0", [(STAGE, we, 1, (3, 0))], sh, 1, K=147))
    ls = []
    for lvl in range(2):
        for c in range(LEVELS[lvl]):
            q = f"{b}.level{lvl}."
            x = conv_bn_relu(q + str(3 * c), q + str(3 * c + 1), x, 2 if (c == 0 and lvl == 1) else 1)
        ls.append(x)
    for lvl in range(2, 6):
        x = tree(f"{b}.level{lvl}", x, LEVELS[lvl], 2, CHANNELS[lvl - 1], CHANNELS[lvl], lvl >= 3, [])
        ls.append(x)
    out = [ls[-1]]
    n = len(ls)
    for i in range(n - 2 - 1):
        ida(f"model.dla_up.ida_{i}", ls, n - i - 2, n, CHANNELS[n - i - 2])
        out.insert(0, ls[-1])
    y = out[:3]
    ida("model.ida_up", y, 0, 3, CHANNELS[2])
    cur = y[-1]
    nh = 0
    while f"model.{nh}.0.weight" in sd:
        nh += 1
    w1 = torch.cat([sd[f"model.{h}.0.weight"].double() for h in range(nh)], 0)
    b1 = torch.cat([sd[f"model.{h}.0.bias"].double() for h in range(nh)], 0)
    hid = _conv(HEADS_HIDDEN, [(cur, w1, 1, 1)], b1, 1)
    hid.hi_lo = True  # where conv3x3 EPI 1 takes the 1x1 heads, it feeds them the fp32 activation as hi + lo
    hid = add(hid)
    w2s = [sd[f"model.{h}.2.weight"].double() for h in range(nh)]
    hc = w2s[0].shape[1]
    ctot = sum(w.shape[0] for w in w2s)
    cpad = (ctot + 3) // 4 * 4
    w2 = torch.zeros((cpad, nh * hc, 1, 1), dtype=torch.float64)
    b2 = torch.zeros(cpad, dtype=torch.float64)
    r0 = 0
    for h, w in enumerate(w2s):  # block diagonal: head h reads its own hidden channels
        w2[r0:r0 + w.shape[0], h * hc:(h + 1) * hc] = w
        b2[r0:r0 + w.shape[0]] = sd[f"model.{h}.2.bias"].double()
        r0 += w.shape[0]
    add(_conv(HEADS_OUT, [(hid, w2, 1, 0)], b2, 0, out_f32=True, K=hc))
    return layers


def up_geometry(layer, xs):
    """(source h, w, target H, W, sy, sx) of a dwconvt layer: planner_dla34.cpp ida()."""
    f = layer.f
    h, w = xs[layer.srcs[0]].shape[2:]
    tH, tW = xs[layer.srcs[1]].shape[2:]
    hu, wu = (h - 1) * f - 2 * (f // 2) + 2 * f, (w - 1) * f - 2 * (f // 2) + 2 * f
    return h, w, tH, tW, max(0, (hu - tH) // 2), max(0, (wu - tW) // 2)


# ---- DCNv2 sampling with its intermediate values ----

def dcn_cols(x, om, fault=None):
    """The modulated deformable sampling of ref_dla34.deform_conv2d (3x3, stride 1, pad 1) in the dtype
    of x: col [B, C, 9, H, W] = m_k * bilinear(x; py, px), and the scales of the bound: m [B, 9, H, W],
    Uabs = sum_corner wt |v|, csum = sum_corner |v| (valid corners), pmax = max(|py|, |px|).
    fault (tests): {"swap_tap": k} dy / dx of tap k swapped; {"mask_shift": 1} mask logits one channel off;
    {"strict": True} samples with -1 < py < 0 treated as outside; {"transpose": True} tap k at (k % 3, k / 3)."""
    fault = fault or {}
    B, C, H, W = x.shape
    dt = x.dtype
    off = om[:, :18].reshape(B, 9, 2, H, W)
    dy, dx = off[:, :, 0], off[:, :, 1]
    if "swap_tap" in fault:
        k = fault["swap_tap"]
        dy, dx = dy.clone(), dx.clone()
        dy[:, k], dx[:, k] = off[:, k, 1], off[:, k, 0]
    s = fault.get("mask_shift", 0)
    logit = om[:, 18 + s:27 + s]
    m = 1.0 / (1.0 + torch.exp(-logit))
    k = torch.arange(9)
    ky, kx = (k % 3, k // 3) if fault.get("transpose") else (k // 3, k % 3)
    py = (torch.arange(H).view(1, 1, H, 1) - 1 + ky.view(1, 9, 1, 1)).to(dt) + dy
    px = (torch.arange(W).view(1, 1, 1, W) - 1 + kx.view(1, 9, 1, 1)).to(dt) + dx
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    if fault.get("strict"):
        inside = inside & (py >= 0)
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    hy, hx = 1 - ly, 1 - lx
    y0i, x0i = y0.long(), x0.long()
    flat = x.reshape(B, C, H * W)
    val = torch.zeros((B, C, 9, H, W), dtype=dt)
    uabs, csum = torch.zeros_like(val), torch.zeros_like(val)
    for cy, cx, wgt in ((0, 0, hy * hx), (0, 1, hy * lx), (1, 0, ly * hx), (1, 1, ly * lx)):
        yy, xx = y0i + cy, x0i + cx
        ok = inside & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(B, 1, 9 * H * W).expand(B, C, 9 * H * W)
        v = torch.gather(flat, 2, idx).view(B, C, 9, H, W)
        okf = ok.to(dt).unsqueeze(1)
        wk = wgt.unsqueeze(1) * okf
        val = val + wk * v
        uabs = uabs + wk * v.abs()
        csum = csum + okf * v.abs()
    pmax = torch.maximum(py.abs(), px.abs())
    return m.unsqueeze(1) * val, m, uabs, csum, pmax


def _dcol(m, uabs, csum, pmax):
    """The sampling error bound per column element [B, C, 9, H, W] (module docstring)."""
    m = m.unsqueeze(1)
    D = 2.0 * 2.0 ** -23 * (pmax.unsqueeze(1) + 1.0) * csum
    return m * uabs * 9 * 2.0 ** -24 * (1 + 2.0 ** -20) + SIG_BAR * uabs + m * D


def _cols_nchw(col):
    """[B, C, 9, H, W] -> the engine's column tensor as NCHW [B, 9 C, H, W], channel k C + c."""
    B, C, _, H, W = col.shape
    return col.permute(0, 2, 1, 3, 4).reshape(B, 9 * C, H, W)


def _gemm_conv(layer):
    """The column GEMM as a 1x1 conv over the stored column tensor (channel k C + c)."""
    if not hasattr(layer, "_gemm"):
        N, C = layer.w.shape[:2]
        w = layer.w.reshape(N, C, 9).permute(0, 2, 1).reshape(N, 9 * C, 1, 1)
        layer._gemm = _conv(layer.label, [(layer.col, w.contiguous(), 1, 0)], layer.bias, 1)
    return layer._gemm


def _contract(w, col):
    N, C = w.shape[:2]
    return torch.einsum("nck,bckhw->bnhw", w.reshape(N, C, 9), col)


def _dwconvt(x, w, f, skip):
    up = F.conv_transpose2d(x, w, None, stride=f, padding=f // 2, groups=w.shape[0])
    return pad_to_match(up, skip.shape)


# ---- one layer ----

def evaluate(layer, xs):
    """The layer in the dtype of its inputs (float64: the reference)."""
    k = layer.kind
    if k in ("conv", "stage"):
        return YL.evaluate(layer, xs)
    x = xs[layer.srcs[0]]
    if k == "maxpool":
        return F.max_pool2d(x, 2, 2, ceil_mode=True)
    if k == "dwconvt":
        skip = xs[layer.srcs[1]]
        return _dwconvt(x, layer.w.to(x.dtype), layer.f, skip) + skip
    om = xs[layer.srcs[1]]
    if k == "dcn_sample":
        return _cols_nchw(dcn_cols(x, om)[0])
    if k == "dcn":
        m = 1.0 / (1.0 + torch.exp(-om[:, 18:27]))
        return F.relu(ref_dla34.deform_conv2d(x, om[:, :18], m, layer.w.to(x.dtype), layer.bias.to(x.dtype), 1, 1))
    raise ValueError(k)


def emulate(layer, xs, precision, fault=None):
    """The reference arithmetic of a correct kernel (module docstring, per kind): stored inputs, weights
    rounded, fp32 accumulation, one output rounding; float64 result. fault: dcn_cols's, for the tests."""
    dt = LR.TORCH_DTYPE[precision]
    k = layer.kind

    def q(t):
        return t.to(dt).double()
    if k in ("conv", "stage"):
        return YL.emulate(layer, xs, precision)
    x = xs[layer.srcs[0]].float()
    if k == "maxpool":
        return evaluate(layer, xs)
    if k == "dwconvt":  # (stored values and fp32 weights summed in fp64, rounded to fp32, then to the dtype)
        skip = xs[layer.srcs[1]].float().double()
        return q((_dwconvt(x.double(), layer.w.float().double(), layer.f, skip) + skip).float())
    om = xs[layer.srcs[1]].float()
    if k == "dcn_sample":
        return q(_cols_nchw(dcn_cols(x, om, fault)[0]))
    if k == "dcn":
        col = dcn_cols(x, om, fault)[0].to(dt).float()
        y = _contract(layer.w.float().to(dt).float(), col) + layer.bias.float().view(1, -1, 1, 1)
        return q(F.relu(y))
    raise ValueError(k)


def bounds(layer, xs, ref, precision, pend=None):
    """(deterministic bound, statistical scale) per element; pend as yolact_layer_ref.bounds."""
    pend = pend or {}
    u, eta = U[precision], ETA[precision]
    uo = 0.0 if precision == "fp32" else u  # a rounding to the compute dtype (fp32: none)
    k = layer.kind
    if k in ("conv", "stage"):
        return YL.bounds(layer, xs, ref, precision, pend)
    aref = ref.abs()
    if k == "maxpool":
        src = layer.srcs[0]
        if src in pend:
            return (F.max_pool2d(pend[src][0], 2, 2, ceil_mode=True), F.max_pool2d(pend[src][1], 2, 2, ceil_mode=True))
        return torch.zeros_like(ref), torch.zeros_like(ref)
    assert not any(s in pend for s in layer.sources()), (layer.label, "reads an unstored tensor")
    x = xs[layer.srcs[0]]
    if k == "dwconvt":
        skip = xs[layer.srcs[1]]
        A = _dwconvt(x.abs(), layer.w.abs(), layer.f, skip) + skip.abs()
        e64 = 10 * 2.0 ** -53 * A
        det = e64 + (2.0 ** -24 + uo * (1 + 2.0 ** -24)) * (aref + e64) + eta
        return det, (uo if uo else u) * aref + eta
    col, m, uabs, csum, pmax = dcn_cols(x, xs[layer.srcs[1]])
    dcol = _dcol(m, uabs, csum, pmax)
    if k == "dcn_sample":
        d = _cols_nchw(dcol)
        return d * (1 + uo) + uo * aref + (eta if uo else 0.0), d + u * aref + eta
    if k == "dcn":
        wa = layer.w.abs()
        A, S = _contract(wa, col.abs()), _contract(wa, dcol)
        Q = torch.sqrt(_contract(layer.w * layer.w, col * col))
        det = (2 * uo * (1 + uo) + layer.K * 2.0 ** -24) * (A + S) + S + u * aref + eta
        return det, u * (aref + 2.0 ** 0.5 * Q) + S + eta
    raise ValueError(k)


def check(layers, img, precision, stored, kernels=None):
    """Teacher-forced per-layer comparison. img: float64 NCHW image; stored: {label: float64 NCHW tensor the
    engine stored for that op, or None}. Returns a LayerReport with one row per judged layer (c for
    LayerReport.failures: C_STAT_DLA34) and .up: {label: (h, w, tH, tW, sy, sx)} of the dwconvt layers."""
    missing = [k for k in layers if k not in stored]
    extra = [k for k in stored if k not in layers]
    assert not missing and not extra, f"no engine op with the labels {missing}; no layer for the engine's ops {extra}"
    kernels = kernels or {}
    vals, pend = {IMG: img}, {}
    rep = LayerReport()
    rep.up = {}
    for label, layer in layers.items():
        got = stored[label]
        kern = kernels.get(label, "")
        if layer.kind == "dcn" and stored[layer.col] is not None:
            layer = _gemm_conv(layer)  # the columns are stored: a plain 1x1 conv over them
        elif layer.kind == "dcn_sample" and got is None:
            vals[label] = None  # sampled inside the fused kernel: judged with the GEMM row
            rep.skipped.append(label)
            continue
        xs = {s: vals[s] for s in layer.sources()}
        ref = evaluate(layer, xs)
        det, stat = bounds(layer, xs, ref, precision, pend)
        r = 2 if layer.kind == "dcn" else 1 + int(any(s in pend for s in layer.sources()))
        if layer.kind == "dwconvt":
            rep.up[label] = up_geometry(layer, xs)
        if got is None:
            pend[label] = YL.pending(layer, ref, det, stat, precision)
            vals[label] = ref
            rep.skipped.append(label)
            continue
        assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
        if getattr(layer, "zero_cols", None):
            assert float(got[:, layer.zero_cols:].abs().max()) == 0.0, f"{label}: padding columns are not exact zeros"
        rd, rs = ratios(got, ref, det, stat)
        idx = tuple(int(v) for v in np.unravel_index(int(torch.argmax(rd)), tuple(rd.shape)))
        rep.rows.append((label, kern, r, float(rd.max()), float(rs.max()), idx, YL._tile(kern, idx, layer, xs)))
        vals[label] = got
    assert len(rep.rows) + len(rep.skipped) == len(layers)
    return rep


def forward(layers, img, step):
    """Every layer by step(layer, xs), without forcing: {label: tensor}."""
    vals = {IMG: img}
    for label, layer in layers.items():
        vals[label] = step(layer, {s: vals[s] for s in layer.sources()})
    return vals


def forward64(layers, img):
    return forward(layers, img, evaluate)


def emulated_forward(layers, img, precision):
    """The whole forward in the reference arithmetic (the CPU stand-in for the engine's stored tensors):
    {label: float64 tensor or None}; the 16-bit plans keep no column tensor (None), the fp32 plan does."""
    vals = forward(layers, img.float().double(), lambda layer, xs: emulate(layer, xs, precision))
    return {k: (None if layers[k].kind == "dcn_sample" and precision != "fp32" else vals[k]) for k in layers}


# ---- the cases of tests/test_gpu_dla34_layers.py ----

# image (h, w, B): module docstring of tests/test_gpu_dla34_layers.py
GEOMETRIES = {"G1": (100, 140, 3), "G1T": (140, 100, 2), "G2": (148, 76, 1), "G3": (36, 44, 5), "G4": (100, 104, 1)}
# what the issue's table names: the five map sizes below the input, and the f = 4 step's (sy, sx)
MAPS = {100: (50, 25, 13, 7, 4), 140: (70, 35, 18, 9, 5), 148: (74, 37, 19, 10, 5), 76: (38, 19, 10, 5, 3),
        104: (52, 26, 13, 7, 4), 36: (18, 9, 5, 3, 2), 44: (22, 11, 6, 3, 2)}
SHIFT_F4 = {"G1": (1, 0), "G1T": (0, 1), "G4": (1, 1)}
N_LABELS = 4


def reference_keys():
    """The reference's state-dict key list for the plain 4-label heads [4, 2, 2] (tests/golden/models_dla34.json)."""
    from helpers import dla34_index
    return [(k, tuple(s)) for k, s in dla34_index()["b2_64x96"]["keys"]]


def seeded_weights():
    """(seeded state dict as loaded, its float64 copy)."""
    from recipe import seeded_state_dict
    sd = seeded_state_dict(reference_keys(), conv_seed=34, aux_seed=35)
    return sd, YL.f64(sd)


def make_model(precision):
    """tv.CenterpointDLA34 with the plain 4-label heads and the seeded weights, on the CPU."""
    import tauv_vision_amd as tv
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(False, 1.0), A(False, 1.0), A(False, 1.0), False, False, None)
                             for i in range(N_LABELS)])
    model = tv.CenterpointDLA34(oc, precision=precision)
    model.load_state_dict(seeded_weights()[0])
    return model.eval()


def oracle_heads(sd64, img):
    """The un-hooked float64 oracle: the head outputs concatenated, NCHW."""
    ref = {k[len("model."):]: v for k, v in sd64.items()}
    nh = 0
    while f"{nh}.0.weight" in ref:
        nh += 1
    with torch.no_grad():
        return torch.cat(ref_dla34.dlaseg_forward(ref, img, nh), 1)
