"""The per-layer method for the YOLACT plans (tests/yolact_layer_ref.py) tested on the CPU: no GPU and no
engine, but the built library, which names the head's parameters (param_layout), as tests/test_host_cpu.py.

1. The graphs (one Layer per engine op, restated from planner_resnet.cpp, planner_yolact_head.cpp and
   planner_protonet.cpp), evaluated in float64 without forcing, are tests/resnet18_ref.py (the taps) and
   tests/yolact_head_ref.py (FPN levels, classification, boxes, mask coefficients, prototypes) to
   1e-9 max(1, |ref|max) on every geometry of tests/test_gpu_yolact_layers.py, n_ar = 2 included (H1,
   the whole model), where the ratio-inner row order matters, and on golden case B for the graph's
   unstacked head branch (branch blocks, three aspect ratios).
2. The emulated forward (the reference arithmetic per layer, fp16 / bf16 / fp32) stays within the
   deterministic bound on every layer of every GPU case, and its largest statistical ratio is the
   constant c of this graph (yolact_layer_ref.C_MEASURED_YOLACT, re-measured here on every run within
   5 %, recorded under "yolact_layers/cpu/<precision>"): fp16 1.92, bf16 2.03. The GPU tests assert
   twice that (3.84 and 4.06). It measures the reference arithmetic only.
3. Seven injected faults, each into the emulation's output of one real layer, break both bounds at
   the elements they touch while the others stay inside:
     (a) the stride-2 `downsample` residual read at stride 1, and one pixel off, at an odd input size
         (layer3.0: 25x35 -> 13x18);
     (b) the BatchNorm scale of the identity segment left out for one 32-channel block (the head
         block's last GEMM);
     (c) the identity residual dropped on the partial last tile row (layer1.0, 50 rows, 16-row tiles);
     (d) the bilinear second tap not clamped on the last row / column, at 7 -> 13 and 9 -> 18;
     (e) two convt3 output phases swapped, and the output one column off;
     (f) head_scatter rows ratio-major instead of pixel-major, with n_ar = 2;
     (g) the last k-step (64 channels of the last tap) of a 512-channel layer4 conv dropped.
   So tests/test_gpu_yolact_layers.py fails for the faults it exists to catch.
"""
import functools

import pytest
import torch

import layer_ref as LR
import resnet18_ref as rr
import yolact_head_ref as yr
import yolact_layer_ref as YL
from helpers import record_measurement

TILE_H = 16


def _close(got, ref, what):
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = float((got - ref).abs().max())
    assert err <= 1e-9 * max(1.0, float(ref.abs().max())), (what, err)


@functools.lru_cache(maxsize=None)
def _backbone(name, B=None):
    _, sd, img = YL.backbone_case(name, B)
    return sd, img.double(), YL.resnet18_layers(sd)


@functools.lru_cache(maxsize=None)
def _head(name, B=None):
    c, _, sd, maps = YL.head_case(name)
    maps = [m[:B or c["batch"]].double() for m in maps]
    layers, lv, proto = YL.yolact_head_layers(sd, 3, c["down"], c["layers"], len(c["ars"]))
    return c, sd, {f"map{i}": m for i, m in enumerate(maps)}, layers, lv, proto


@functools.lru_cache(maxsize=None)
def _whole():
    c, _, sd, img = YL.whole_case()
    layers, lv, proto = YL.yolact_layers(sd, c["down"], c["layers"], len(c["ars"]))
    return c, sd, img.double(), layers, lv, proto


def _check_head_outputs(c, sd, maps, vals, heads, lv, proto):
    with torch.no_grad():
        cls, box, coef, pr, fpn = yr.yolact_head(sd, maps, c["C"], c["k"])
    for i, (label, f) in enumerate(zip(lv, fpn)):
        _close(vals[label], f, f"fpn{i}")
    assert len(lv) == len(fpn)
    _close(heads[0], cls, "classification")
    _close(heads[1], box, "box_encoding")
    _close(heads[2], coef, "mask_coeff")
    _close(vals[proto][:, :c["k"]], pr, "mask_prototype")
    assert float(vals[proto][:, c["k"]:].abs().sum()) == 0.0  # (the columns up to a multiple of 4)


# ---- 1. the graphs are the restatements ----

@pytest.mark.parametrize("name", list(YL.BACKBONE_GEOMETRIES))
def test_backbone_graph_is_the_restatement(name):
    sd, img, (layers, taps) = _backbone(name)
    with torch.no_grad():
        want = rr.resnet18_ref(sd)(img)
        vals, heads = YL.forward64(layers, {YL.IMG: img})
    assert heads is None and len(taps) == 3
    for i, (t, w) in enumerate(zip(taps, want)):
        _close(vals[t], w, f"{name} tap {i}")
        _close(vals[f"layer{i + 2}.1.bn2 -> fp32 NHWC"], w, f"{name} stored tap {i}")


@pytest.mark.parametrize("name", list(YL.HEAD_GEOMETRIES))
def test_head_graph_is_the_restatement(name):
    c, sd, inputs, layers, lv, proto = _head(name)
    with torch.no_grad():
        vals, heads = YL.forward64(layers, inputs)
        _check_head_outputs(c, sd, [inputs[f"map{i}"] for i in range(3)], vals, heads, lv, proto)


def test_unstacked_head_graph_is_the_restatement():
    """Golden case B (branch blocks: three final convs of their own, three aspect ratios): the graph's
    other head branch, which no GPU geometry of this file takes."""
    from recipe_yolact_head import head_case, head_inputs
    c = head_case("yolact_head_b")
    sd, maps = head_inputs(c)
    sd, maps = YL.f64(sd), [m.double() for m in maps]
    layers, lv, proto = YL.yolact_head_layers(sd, 3, c["down"], c["layers"], len(c["ars"]))
    assert not any("(stacked)" in k for k in layers)
    with torch.no_grad():
        vals, heads = YL.forward64(layers, {f"map{i}": m for i, m in enumerate(maps)})
        _check_head_outputs(c, sd, maps, vals, heads, lv, proto)


def test_whole_model_graph_is_the_restatements():
    c, sd, img, layers, lv, proto = _whole()
    with torch.no_grad():
        bb = rr.resnet18_ref({k[len(YL.BB):]: v for k, v in sd.items() if k.startswith(YL.BB)})
        taps = list(bb(img))
        vals, heads = YL.forward64(layers, {YL.IMG: img})
        _check_head_outputs(c, {k: v for k, v in sd.items() if not k.startswith(YL.BB)}, taps, vals, heads, lv, proto)
    assert YL.BB + "layer4.1.conv2 + bn2 (tap)" in layers and "layer4.1.bn2 -> fp32 NHWC" not in layers


def test_bilinear_by_gathers_is_interpolate():
    g = torch.Generator().manual_seed(3)
    for src, dst in (((7, 9), (13, 18)), ((4, 5), (7, 9)), ((13, 18), (25, 35)), ((1, 1), (2, 2))):
        x = torch.randn((2, 3, *src), generator=g, dtype=torch.float64)
        _close(YL.bilinear(x, dst), torch.nn.functional.interpolate(x, dst, mode="bilinear"), (src, dst))


# ---- 2. the emulated forward: inside the deterministic bound, and c ----

def _cases():
    for name in YL.BACKBONE_GEOMETRIES:
        sd, img, (layers, _) = _backbone(name)
        yield name, layers, {YL.IMG: img}
    for name in YL.HEAD_GEOMETRIES:
        _, _, inputs, layers, _, _ = _head(name)
        yield name, layers, inputs
    _, _, img, layers, _, _ = _whole()
    yield "W", layers, {YL.IMG: img}


@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_emulation_within_bounds_and_measures_c(precision):
    worst_det, worst_stat, tanh = 0.0, 0.0, 0.0
    for name, layers, inputs in _cases():
        if precision == "fp32" and name not in ("R2", "H1"):  # (the fp32 GPU cases)
            continue
        with torch.no_grad():
            stored, heads = YL.emulated_forward(layers, inputs, precision)
            rep = YL.check(layers, inputs, precision, stored, heads=heads)
        n_phase = sum(l.kind == "phase" for l in layers.values())
        n_scatter = sum(l.kind == "head_scatter" for l in layers.values())
        assert len(rep.skipped) == n_phase and len(rep.rows) == len(layers) - n_phase
        d, s = rep.worst()
        print(f"{name} {precision}: {d:.3f} x deterministic, {s:.3f} x u(|ref|+Q), tanh {rep.tanh_err:.2e}, "
              f"{len(rep.rows)} layers ({n_scatter} scatters)")
        if precision == "fp32":
            bad = [r for r in rep.rows if r[3] > 1.0]
            assert not bad, bad
        else:
            fails = rep.failures(YL.C_STAT_YOLACT[precision])
            assert not fails, "\n".join(fails)
        worst_det, worst_stat, tanh = max(worst_det, d), max(worst_stat, s), max(tanh, rep.tanh_err)
    record_measurement(f"yolact_layers/cpu/{precision}", {"max_det_ratio": worst_det, "c_measured": worst_stat,
                                                          "tanh_err": tanh})
    if precision != "fp32":
        # C_MEASURED_YOLACT is this number (the fp32 summation order of the host's convolution may move it a little)
        c = YL.C_MEASURED_YOLACT[precision]
        assert abs(worst_stat - c) <= 0.05 * c, worst_stat


# ---- 3. injected faults, one layer at a time (R1 and H1 at B = 1) ----

@functools.lru_cache(maxsize=None)
def _r1(precision):
    sd, img, (layers, _) = _backbone("R1", 1)
    with torch.no_grad():
        vals, _ = YL.emulated_forward(layers, {YL.IMG: img}, precision)
    return layers, dict(vals, **{YL.IMG: img})


@functools.lru_cache(maxsize=None)
def _h1(precision):
    _, _, inputs, layers, _, _ = _head("H1", 1)
    with torch.no_grad():
        vals, heads = YL.emulated_forward(layers, inputs, precision)
    return layers, dict(vals, **inputs), heads


def _judge(layer, xs, got, precision):
    ref = YL.evaluate(layer, xs)
    det, stat = YL.bounds(layer, xs, ref, precision)
    return YL.ratios(got, ref, det, stat)


def _assert_fault(layer, xs, good, bad, touched, precision):
    """`bad` differs from `good` only where `touched`; good passes, bad breaks both bounds there."""
    c = YL.C_STAT_YOLACT[precision]
    rd, rs = _judge(layer, xs, good, precision)
    assert float(rd.max()) <= 1.0 and float(rs.max()) <= c, (float(rd.max()), float(rs.max()))
    assert torch.equal(bad[~touched], good[~touched])
    rd, rs = _judge(layer, xs, bad, precision)
    assert float(rd[touched].max()) > 1.0, float(rd[touched].max())
    assert float(rs[touched].max()) > c, float(rs[touched].max())
    if bool((~touched).any()):
        assert float(rd[~touched].max()) <= 1.0 and float(rs[~touched].max()) <= c
    print(f"{layer.label} {precision}: {float(rd[touched].max()):.3g} x deterministic, "
          f"{float(rs[touched].max()):.3g} x u(|ref|+Q)")


def _xs(layer, vals):
    return {s: vals[s] for s in layer.sources()}


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("how", ["stride 1", "one pixel off"])
def test_downsample_residual_misread_breaks_the_bounds(how, precision):
    """(a)"""
    layers, vals = _r1(precision)
    layer = layers["layer3.0.conv2 + bn2 + downsample + ReLU"]
    xs = _xs(layer, vals)
    (h, w2, _, _), (src, wd, stride, _) = layer.segs
    x = xs[src]
    assert stride == 2 and tuple(x.shape[2:]) == (25, 35)
    good = YL.emulate(layer, xs, precision)
    Ho, Wo = good.shape[2:]
    z = torch.zeros_like(x)  # read at stride 2, z gives what the fault reads
    touched = torch.ones_like(good, dtype=torch.bool)
    if how == "stride 1":
        z[:, :, ::2, ::2] = x[:, :, :Ho, :Wo]
        touched[:, :, 0, 0] = False  # (pixel (0, 0) is the same either way)
    else:
        z[:, :, 0:-1:2, 0:-1:2] = x[:, :, 1::2, 1::2]
    broken = YL._conv(layer.label, [(h, w2, 1, 1), ("misread", wd, 2, 0)], layer.bias, layer.act)
    bad = YL.emulate(broken, dict(xs, misread=z), precision)
    bad[~touched] = good[~touched]
    _assert_fault(layer, xs, good, bad, touched, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_identity_bn_scale_left_out_breaks_the_bounds(precision):
    """(b)"""
    layers, vals, _ = _h1(precision)
    layer = layers["level 0 _prediction_head._extra_conv_layers.0 + _extra_bn_layers.0(bottleneck)"]
    xs = _xs(layer, vals)

    def unscaled(i, w):
        if i == 1:
            w = w.clone()
            w[32:64, 32:64] = torch.eye(32).view(32, 32, 1, 1)
        return w
    good = YL.emulate(layer, xs, precision)
    bad = LR.emulate(layer, xs, precision, weight_fault=unscaled)
    touched = torch.zeros_like(good, dtype=torch.bool)
    touched[:, 32:64] = True
    _assert_fault(layer, xs, good, bad, touched, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_identity_residual_dropped_on_last_tile_row_breaks_the_bounds(precision):
    """(c)"""
    layers, vals = _r1(precision)
    layer = layers["layer1.0.conv2 + bn2 + x + ReLU"]
    xs = _xs(layer, vals)
    good = YL.emulate(layer, xs, precision)
    assert good.shape[2] == 50 and good.shape[2] % TILE_H
    y0 = (good.shape[2] - 1) // TILE_H * TILE_H
    bad = good.clone()
    bad[:, :, y0:] = LR.emulate(layer, xs, precision, weight_fault=lambda i, w: w * 0 if i == 1 else w)[:, :, y0:]
    touched = torch.zeros_like(good, dtype=torch.bool)
    touched[:, :, y0:] = True
    _assert_fault(layer, xs, good, bad, touched, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_unclamped_bilinear_tap_breaks_the_bounds(precision):
    """(d): 7 -> 13 rows and 9 -> 18 columns: the last row / column has a second tap past the map."""
    layers, vals, _ = _h1(precision)
    layer = layers["pyramid 0 = lateral + bilinear(pyramid 1)"]
    xs = _xs(layer, vals)
    x, lat = xs[layer.srcs[0]], xs[layer.srcs[1]]
    assert tuple(x.shape[2:]) == (7, 9) and tuple(lat.shape[2:]) == (13, 18)
    dt = LR.TORCH_DTYPE[precision]
    good = YL.emulate(layer, xs, precision)
    up = YL.bilinear(x, lat.shape[2:], clamp=False).float().to(dt).float()
    wrong = (lat.float() + up).to(dt).double()
    for sel in ((slice(None), slice(None), -1, slice(0, -1)), (slice(None), slice(None), slice(0, -1), -1)):
        touched = torch.zeros_like(good, dtype=torch.bool)
        touched[sel] = True
        bad = good.clone()
        bad[touched] = wrong[touched]
        _assert_fault(layer, xs, good, bad, touched, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_convt3_phases_swapped_or_shifted_break_the_bounds(precision):
    """(e)"""
    layers, vals, _ = _h1(precision)
    layer = layers["_masknet._upsample_layer_1 phase (0,0) + LeakyReLU"]
    xs = _xs(layer, vals)
    good = YL.emulate(layer, xs, precision)
    assert tuple(good.shape[2:]) == (26, 36)
    bad = good.clone()
    bad[:, :, 0::2, 1::2], bad[:, :, 1::2, 0::2] = good[:, :, 1::2, 0::2], good[:, :, 0::2, 1::2]
    touched = torch.zeros_like(good, dtype=torch.bool)
    touched[:, :, 0::2, 1::2] = touched[:, :, 1::2, 0::2] = True
    _assert_fault(layer, xs, good, bad, touched, precision)
    off = good.clone()
    off[..., 1:] = good[..., :-1]
    c = YL.C_STAT_YOLACT[precision]
    rd, rs = _judge(layer, xs, off, precision)
    # every column written from its neighbour holds elements past both bounds
    assert bool((rd.amax((0, 1, 2))[1:] > 1.0).all()) and bool((rs.amax((0, 1, 2))[1:] > c).all())


def test_head_scatter_ratio_major_rows_break_the_bounds():
    """(f): n_ar = 2. The copy's bound is 0 and the tanh bar 1e-4: rows moved by whole anchors are far outside."""
    layers, vals, heads = _h1("fp16")
    label = "level 0 raw heads -> classification / box_encoding / tanh(mask_coeff)"
    layer = layers[label]
    assert layer.n_ar == 2
    xs = _xs(layer, vals)
    # (a two-op graph: the stored raw tensor as it is, then the scatter)
    graph = {layer.srcs[0]: YL.Op(layer.srcs[0], "store_f32", ["raw"]), label: layer}
    good = YL.emulate(layer, xs, "fp16")
    n = good[0].shape[1]
    for j in range(3):
        assert torch.equal(good[j], heads[j][:, :n])
    raw = xs[layer.srcs[0]]
    B, _, H, W = raw.shape

    def run(blocks):
        rep = YL.check(graph, {"raw": raw}, "fp16", {layer.srcs[0]: raw, label: None}, heads=blocks)
        return rep.rows[-1]
    assert run(good)[3] <= 1.0
    for j, (_, c0, cols, _) in enumerate(layer.parts):
        r = raw[:, c0:c0 + cols]
        if j == 2:
            r = torch.tanh(r.float()).double()
        wrong = r.reshape(B, 2, cols // 2, H * W).permute(0, 1, 3, 2).reshape(B, H * W * 2, cols // 2)
        bad = list(good)
        bad[j] = wrong
        row = run(tuple(bad))
        assert row[3] > 1.0 and row[5][3] == j, row


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_dropped_last_k_step_of_layer4_breaks_the_bounds(precision):
    """(g): the last k-step of the 9 x 512 reduction: 64 channels of tap (2, 2)."""
    layers, vals = _r1(precision)
    layer = layers["layer4.1.conv1 + bn1 + ReLU"]
    xs = _xs(layer, vals)
    assert layer.segs[0][1].shape[1] == 512

    def drop(i, w):
        w = w.clone()
        w[:, 448:, 2, 2] = 0
        return w
    good = YL.emulate(layer, xs, precision)
    bad = good.clone()
    touched = torch.zeros_like(good, dtype=torch.bool)
    touched[:, :, :-1, :-1] = True  # (on the last row / column tap (2, 2) reads the padding)
    bad[touched] = LR.emulate(layer, xs, precision, weight_fault=drop)[touched]
    _assert_fault(layer, xs, good, bad, touched, precision)
