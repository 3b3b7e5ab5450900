"""The per-layer method for the DLA-34 plan (tests/dla34_layer_ref.py) tested on the CPU: no GPU, no engine.

1. The graph (one Layer per engine op, restated from planner_dla34.cpp), evaluated in float64 without
   forcing, is oracle.ref_dla34.dlaseg_forward to 1e-9 max(1, |ref|max) on every geometry of
   tests/test_gpu_dla34_layers.py; dcn_cols(), contracted, is ref_dla34.deform_conv2d; the graph's
   planned map sizes and (sy, sx) of the f = 4 step are the ones the geometries were chosen for.
2. The emulated forward (the reference arithmetic per layer) stays within both bounds on every layer of
   every GPU case, and its largest statistical ratio is the constant c of this graph
   (dla34_layer_ref.C_MEASURED_DLA34, re-measured here on every run within 5 %, recorded under
   "layers/dla34/cpu/<precision>"). The GPU tests assert twice that.
3. Injected faults, each into the emulation's output of one real layer of a geometry where it matters,
   break both bounds:
     (1) root K-segments in another order (children first); the 64-channel segment read at the wrong ci0;
     (2) floor-mode pooling (the over-hanging row and column dropped); a ceil-mode window that reads the
         next row's first pixel instead of stopping at the edge;
     (3) tree1's residual taken from the un-pooled input at stride 2 instead of the pooled bottom;
     (4) the level_root child (the pooled bottom) left out of an outer tree's root;
     (5) the pad_to_match shift on the wrong axis (sy <-> sx, G1: sy = 1, sx = 0); dropped on the f = 4
         step (G4: sy = sx = 1);
     (6) depthwise ConvTranspose taps transposed (ky <-> kx); the p = f / 2 padding off by one;
     (7) DCN: dy / dx swapped for one tap;  (8) mask logits read one channel off;
     (9) samples with -1 < py < 0 treated as outside;  (10) tap k visiting (k % 3, k / 3).
   So tests/test_gpu_dla34_layers.py fails for the faults it exists to catch.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import dla34_layer_ref as DL
import layer_ref as LR
import yolact_layer_ref as YL
from helpers import record_measurement
from oracle import ref_dla34

L3 = "model.base.level3"


@functools.lru_cache(maxsize=None)
def _graph():
    sd = DL.seeded_weights()[1]
    return sd, DL.dla34_layers(sd)


@functools.lru_cache(maxsize=None)
def _img(name, B=None):
    h, w, b0 = DL.GEOMETRIES[name]
    return LR.case_frames(h, w, B or b0)[1].double()


@functools.lru_cache(maxsize=None)
def _emulated(name, precision, B=None):
    _, layers = _graph()
    with torch.no_grad():
        stored = DL.emulated_forward(layers, _img(name, B), precision)
    return stored


@functools.lru_cache(maxsize=None)
def _vals(name, precision):
    """Every emulated tensor of the geometry at B = 1 (the column tensors too), and the image."""
    _, layers = _graph()
    img = _img(name, 1)
    with torch.no_grad():
        vals = DL.forward(layers, img.float().double(), lambda layer, xs: DL.emulate(layer, xs, precision))
    return layers, vals


# ---- 1. the graph is the oracle ----

@pytest.mark.parametrize("name", list(DL.GEOMETRIES))
def test_graph_is_the_oracle(name):
    sd, layers = _graph()
    img = _img(name, 1)
    with torch.no_grad():
        vals = DL.forward64(layers, img)
        want = DL.oracle_heads(sd, img)
    got = vals[DL.HEADS_OUT]
    n = want.shape[1]
    assert got.shape[1] == (n + 3) // 4 * 4 and got.shape[0::2] == want.shape[0::2]
    err = float((got[:, :n] - want).abs().max())
    assert err <= 1e-9 * max(1.0, float(want.abs().max())), err
    assert float(got[:, n:].abs().sum()) == 0.0
    # the planned maps and the f = 4 step's shift are the ones the geometry was chosen for
    h, w, _ = DL.GEOMETRIES[name]
    sizes = {tuple(v.shape[2:]) for k, v in vals.items() if k != DL.IMG}
    for mh, mw in zip(DL.MAPS[h], DL.MAPS[w]):
        assert (mh, mw) in sizes, (name, mh, mw)
    up = layers[DL.UP_F4]
    geo = DL.up_geometry(up, {s: vals[s] for s in up.sources()})
    assert up.f == 4 and geo[:2] == (DL.MAPS[h][3], DL.MAPS[w][3]) and geo[2:4] == (DL.MAPS[h][1], DL.MAPS[w][1])
    if name in DL.SHIFT_F4:
        assert geo[4:] == DL.SHIFT_F4[name], (name, geo)
    om = next(k for k in layers if k.endswith(".offset+mask"))
    assert float(vals[om][:, 27:].abs().max()) == 0.0


def test_graph_labels_and_segments():
    _, layers = _graph()
    assert sum(l.kind == "maxpool" for l in layers.values()) == 4 and DL.MAXPOOL + " #4" in layers
    assert sum(l.kind == "dcn" for l in layers.values()) == 16
    assert sorted(l.f for l in layers.values() if l.kind == "dwconvt") == [2] * 7 + [4]
    assert [s[1].shape[1] for s in layers[L3 + ".tree2.root.conv"].segs] == [128, 128, 64, 128]
    assert [s[1].shape[1] for s in layers["model.base.level5.root.conv"].segs] == [512, 512, 256]
    t2 = layers[L3 + ".tree2.tree1.conv2+residual"]  # stride 1, cin == cout: an identity over the tree's input
    assert t2.exact == {t2.segs[1][0]} and t2.segs[1][0] == L3 + ".tree1.root.conv"
    assert DL.unique_labels(["a", "b", "a", "a"]) == ["a", "b", "a #2", "a #3"]


def test_dcn_cols_contracted_is_deform_conv2d():
    g = torch.Generator().manual_seed(4)
    x = torch.randn((2, 8, 7, 5), generator=g, dtype=torch.float64)
    om = torch.randn((2, 32, 7, 5), generator=g, dtype=torch.float64) * 1.5  # offsets past the borders too
    w = torch.randn((6, 8, 3, 3), generator=g, dtype=torch.float64)
    b = torch.randn(6, generator=g, dtype=torch.float64)
    col, m, uabs, csum, pmax = DL.dcn_cols(x, om)
    want = ref_dla34.deform_conv2d(x, om[:, :18], torch.sigmoid(om[:, 18:27]), w, b, 1, 1)
    got = DL._contract(w, col) + b.view(1, -1, 1, 1)
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())
    assert bool((col.abs() <= m.unsqueeze(1) * uabs + 1e-12).all()) and bool((uabs <= csum + 1e-12).all())
    layer = YL.Op("dcn", "dcn", ["x", "om"], col="c", w=w, bias=b, K=72)
    gemm = DL._gemm_conv(layer)  # the column tensor's channel order is the GEMM's
    y = LR.evaluate(gemm, {"c": DL._cols_nchw(col)})
    assert float((y - F.relu(want)).abs().max()) <= 1e-9 * float(want.abs().max())


# ---- 2. the emulated forward: inside both bounds, and c ----

@pytest.mark.parametrize("precision", ["fp16", "bf16", "fp32"])
def test_emulation_within_bounds_and_measures_c(precision):
    _, layers = _graph()
    worst_det = worst_stat = 0.0
    for name in DL.GEOMETRIES:
        if precision == "fp32" and name not in ("G2", "G4"):  # (the fp32 GPU cases)
            continue
        stored = _emulated(name, precision)
        with torch.no_grad():
            rep = DL.check(layers, _img(name), precision, stored)
        n_cols = sum(l.kind == "dcn_sample" for l in layers.values())
        assert len(rep.skipped) == (0 if precision == "fp32" else n_cols)
        d, s = rep.worst()
        mm = max(r[4] for r in rep.rows if layers[r[0]].kind in ("conv", "dcn"))
        print(f"{name} {precision}: {d:.3f} x deterministic, {s:.3f} x statistical scale (matrix ops {mm:.3f}), "
              f"{len(rep.rows)} layers")
        if precision == "fp32":
            bad = [r for r in rep.rows if r[3] > 1.0]
            assert not bad, bad
        else:
            fails = rep.failures(DL.C_STAT_DLA34[precision])
            assert not fails, "\n".join(fails)
        worst_det, worst_stat = max(worst_det, d), max(worst_stat, s)
    record_measurement(f"layers/dla34/cpu/{precision}", {"max_det_ratio": worst_det, "c_measured": worst_stat})
    if precision != "fp32":
        c = DL.C_MEASURED_DLA34[precision]
        assert abs(worst_stat - c) <= 0.05 * c, worst_stat


# ---- 3. injected faults ----

def _judge(layer, xs, got, precision):
    ref = DL.evaluate(layer, xs)
    det, stat = DL.bounds(layer, xs, ref, precision)
    return DL.ratios(got, ref, det, stat)


def _assert_fault(layer, xs, good, bad, precision, touched=None):
    """good passes both bounds; bad breaks both (where `touched`, and nowhere else)."""
    c = DL.C_STAT_DLA34[precision]
    rd, rs = _judge(layer, xs, good, precision)
    assert float(rd.max()) <= 1.0 and float(rs.max()) <= c, (float(rd.max()), float(rs.max()))
    assert bad.shape == good.shape
    rd, rs = _judge(layer, xs, bad, precision)
    if touched is None:
        touched = torch.ones_like(good, dtype=torch.bool)
    else:
        assert torch.equal(bad[~touched], good[~touched])
    assert float(rd[touched].max()) > 1.0, float(rd[touched].max())
    assert float(rs[touched].max()) > c, float(rs[touched].max())
    print(f"{layer.label} {precision}: {float(rd[touched].max()):.3g} x deterministic, "
          f"{float(rs[touched].max()):.3g} x statistical scale")


def _xs(layer, vals):
    return {s: vals[s] for s in layer.sources()}


def _conv_like(layer, segs):
    return YL._conv(layer.label, segs, layer.bias, layer.act)


PREC = pytest.mark.parametrize("precision", ["fp16", "bf16"])


@PREC
@pytest.mark.parametrize("how", ["children first", "wrong ci0"])
def test_root_segments_misordered_break_the_bounds(how, precision):
    """(1): level 3's outer root, 128 + 128 + 64 + 128."""
    layers, vals = _vals("G4", precision)
    layer = layers[L3 + ".tree2.root.conv"]
    xs = _xs(layer, vals)
    good = DL.emulate(layer, xs, precision)
    srcs = [s[0] for s in layer.segs]
    assert [vals[s].shape[1] for s in srcs] == [128, 128, 64, 128]
    if how == "children first":
        cat = torch.cat([vals[s] for s in srcs[2:] + srcs[:2]], 1)
        broken = _conv_like(layer, [("cat", layer.w_full, 1, 0)])
        bad = DL.emulate(broken, {"cat": cat}, precision)
    else:  # the pooled bottom's 64 channels read against weight columns 0..63 instead of 256..319
        segs = list(layer.segs)
        segs[2] = (srcs[2], layer.w_full[:, 0:64], 1, 0)
        bad = DL.emulate(_conv_like(layer, segs), xs, precision)
    _assert_fault(layer, xs, good, bad, precision)


@PREC
@pytest.mark.parametrize("how", ["floor mode", "reads the next row"])
def test_pooling_edge_faults_break_the_bounds(how, precision):
    """(2): 25x26 -> 13x13 (G4, odd height) and 25x35 -> 13x18 (G1, odd both ways)."""
    for name in ("G4", "G1"):
        layers, vals = _vals(name, precision)
        layer = layers[DL.MAXPOOL + " #2"]
        xs = _xs(layer, vals)
        x = xs[layer.srcs[0]]
        H, W = x.shape[2:]
        assert H == 25 and W in (26, 35)
        good = DL.emulate(layer, xs, precision)
        bad = good.clone()
        touched = torch.zeros_like(good, dtype=torch.bool)
        if how == "floor mode":  # the over-hanging windows are never written: the tensor keeps its zeros
            touched[:, :, -1, :] = True
            if W % 2:
                touched[:, :, :, -1] = True
            bad[touched] = 0.0
        else:  # x = W is the flat successor: the next row's first pixel (nothing after the last row)
            if W % 2 == 0:
                continue
            nxt = F.pad(x[:, :, 1:, 0], (0, 1))          # [B, C, H]: x[y + 1, 0]
            pair = torch.maximum(x[..., -1], nxt)        # the window's row y: max(x[y, W - 1], x[y + 1, 0])
            pair = F.pad(pair, (0, 1), value=float("-inf"))
            touched[:, :, :, -1] = True
            bad[:, :, :, -1] = torch.maximum(pair[..., 0::2], pair[..., 1::2])
            touched &= bad != good
        _assert_fault(layer, xs, good, bad, precision, touched)


@PREC
def test_residual_from_the_unpooled_input_breaks_the_bounds(precision):
    """(3): level 3's tree1.tree1 (25x26 -> 13x13): `project` over x[::2, ::2] instead of the pooled bottom."""
    layers, vals = _vals("G4", precision)
    layer = layers[L3 + ".tree1.tree1.conv2+residual"]
    xs = _xs(layer, vals)
    (t, w2, _, _), (bottom, wr, _, _) = layer.segs
    x = layers[bottom].srcs[0]
    assert layers[bottom].kind == "maxpool" and tuple(vals[x].shape[2:]) == (25, 26)
    good = DL.emulate(layer, xs, precision)
    bad = DL.emulate(_conv_like(layer, [(t, w2, 1, 1), (x, wr, 2, 0)]), {t: vals[t], x: vals[x]}, precision)
    _assert_fault(layer, xs, good, bad, precision)


@PREC
def test_level_root_child_left_out_breaks_the_bounds(precision):
    """(4)"""
    layers, vals = _vals("G4", precision)
    layer = layers[L3 + ".tree2.root.conv"]
    xs = _xs(layer, vals)
    assert layers[layer.segs[2][0]].kind == "maxpool"
    good = DL.emulate(layer, xs, precision)
    bad = LR.emulate(layer, xs, precision, weight_fault=lambda i, w: w * 0 if i == 2 else w)
    _assert_fault(layer, xs, good, bad, precision)


def _place(up, tH, tW, sy, sx):
    """The up-sampled map read at (y - sy, x - sx), zero outside it (dla34.hip dwconvt_add)."""
    out = torch.zeros(up.shape[:2] + (tH, tW), dtype=up.dtype)
    hh, ww = min(tH - sy, up.shape[2]), min(tW - sx, up.shape[3])
    out[:, :, sy:sy + hh, sx:sx + ww] = up[:, :, :hh, :ww]
    return out


def _up_emulated(layer, xs, precision, shift=None, w=None, padding=None):
    dt = LR.TORCH_DTYPE[precision]
    x, skip = xs[layer.srcs[0]].float().double(), xs[layer.srcs[1]].float().double()
    f = layer.f
    w = (layer.w.float() if w is None else w).double()
    up = F.conv_transpose2d(x, w, None, stride=f, padding=f // 2 if padding is None else padding, groups=w.shape[0])
    if padding is not None:  # a map smaller by 2 per axis per unit of extra padding, placed as the planner's shift says
        up = F.pad(up, (0, 2 * (padding - f // 2), 0, 2 * (padding - f // 2)))
    _, _, tH, tW, sy, sx = DL.up_geometry(layer, xs)
    sy, sx = (sy, sx) if shift is None else shift
    return (_place(up, tH, tW, sy, sx) + skip).float().to(dt).double()


@PREC
@pytest.mark.parametrize("how", ["wrong axis", "dropped"])
def test_pad_to_match_shift_faults_break_the_bounds(how, precision):
    """(5): the f = 4 step, 7x9 -> 28x36 onto 25x35 (G1: sy = 1, sx = 0) and 7x7 -> 28x28 onto 25x26 (G4: 1, 1)."""
    name = "G1" if how == "wrong axis" else "G4"
    layers, vals = _vals(name, precision)
    layer = layers[DL.UP_F4]
    xs = _xs(layer, vals)
    sy, sx = DL.up_geometry(layer, xs)[4:]
    assert (sy, sx) == DL.SHIFT_F4[name] and layer.f == 4
    good = DL.emulate(layer, xs, precision)
    assert torch.equal(good, _up_emulated(layer, xs, precision))
    bad = _up_emulated(layer, xs, precision, shift=(sx, sy) if how == "wrong axis" else (0, 0))
    _assert_fault(layer, xs, good, bad, precision)


@PREC
@pytest.mark.parametrize("how", ["taps transposed", "padding off by one"])
def test_depthwise_convtranspose_faults_break_the_bounds(how, precision):
    """(6): on the f = 4 step and on an f = 2 step."""
    layers, vals = _vals("G4", precision)
    for label in (DL.UP_F4, "model.ida_up.up_1+pad_to_match+add"):
        layer = layers[label]
        xs = _xs(layer, vals)
        good = DL.emulate(layer, xs, precision)
        if how == "taps transposed":
            bad = _up_emulated(layer, xs, precision, w=layer.w.float().transpose(2, 3).contiguous())
        else:
            bad = _up_emulated(layer, xs, precision, padding=layer.f // 2 + 1)
        _assert_fault(layer, xs, good, bad, precision)


@PREC
@pytest.mark.parametrize("fault", [{"swap_tap": 5}, {"mask_shift": 1}, {"strict": True}, {"transpose": True}],
                         ids=["dy dx swapped", "mask one channel off", "py in (-1, 0) outside", "taps transposed"])
def test_dcn_sampling_faults_break_the_bounds(fault, precision):
    """(7) - (10): on a 64-channel 25x26 layer and on the 512-channel 4x4 one."""
    layers, vals = _vals("G4", precision)
    for label in ("model.ida_up.node_2.conv+actf", "model.dla_up.ida_0.proj_1.conv+actf"):
        layer = layers[label]
        xs = _xs(layer, vals)
        good = DL.emulate(layer, xs, precision)
        bad = DL.emulate(layer, xs, precision, fault)
        touched = None
        if "strict" in fault:  # only windows near the first row have such samples
            touched = bad != good
            assert bool(touched[:, :, 0].any())
        _assert_fault(layer, xs, good, bad, precision, touched)


def test_dcn_sample_row_is_judged_where_the_columns_are_stored():
    """The fp32 plan's two rows: a column tensor off by one tap fails the dcn_sample row's bound."""
    layers, vals = _vals("G4", "fp32")
    label = "model.ida_up.node_2.conv (DCNv2 sampling)"
    layer = layers[label]
    xs = _xs(layer, vals)
    good = DL.emulate(layer, xs, "fp32")
    rd, _ = _judge(layer, xs, good, "fp32")
    assert float(rd.max()) <= 1.0
    rd, _ = _judge(layer, xs, DL.emulate(layer, xs, "fp32", {"swap_tap": 0}), "fp32")
    assert float(rd.max()) > 1.0
