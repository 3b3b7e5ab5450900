"""The per-layer method (tests/layer_ref.py) tested on the CPU: no GPU and no engine, but the built
library, which names the model's parameters (tv.Centernet -> param_layout), as tests/test_host_cpu.py.

For each op kind (3x3 stride 1; 3x3 stride 2 and 3x3 + 1x1 stride-2 residual; Root over a channel
concat; ConvTranspose + pad_to_match + add with the H-excess-pads-W shift and a crop; the stacked
heads + their 1x1 as a fused chain) on real layers of the 100x140 case (25x35 and 13x18 maps):
the reference arithmetic (inputs as stored, weights rounded to the compute dtype, fp32 accumulation,
one output rounding) passes both bounds, and each of three injected faults at an edge breaks both
bounds at the pixels it touches and nowhere else:
  * a halo column read as zero (the column right of a 32-wide tile, as the last column of that tile
    sees it);
  * one 32-channel k-step of one tap dropped on the last partial tile row (16-row tiles);
  * the ConvTranspose target written one column off.
So tests/test_gpu_layers.py fails for the faults it exists to catch.

This is also where the statistical constant c is measured: the largest err / (u (|ref| + Q)) of
the reference arithmetic over every layer of every GPU case. Measured here (and re-measured by
test_emulation_within_bounds_and_measures_c on every run; recorded under "layers/cpu/..."):
fp16 1.96, bf16 2.31 (layer_ref.C_MEASURED; every layer reads its inputs as the oracle does, the stem
the fp32 image); the GPU tests assert twice that, 3.92 and 4.62.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import layer_ref as LR
from helpers import record_measurement
from oracle.ref_forward import HEADS_HIDDEN_LABEL, HEADS_OUT_LABEL, pad_to_match

# (C, in_h, in_w, B) of every GPU case (tests/test_gpu_layers.py: GEOMETRIES, B_4PHASE, the 64-channel leg)
CASES = [(128, 100, 140, 3), (128, 148, 76, 1), (128, 36, 44, 5), (64, 100, 140, 3), (64, 148, 76, 1),
         (64, 36, 44, 5), (128, 100, 140, 18)]


@functools.lru_cache(maxsize=None)
def _model(C):
    return LR.make_model(C, "fp16")[1]


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_emulation_within_bounds_and_measures_c(precision):
    worst_det, worst_stat = 0.0, 0.0
    for C, h, w, B in CASES:
        if B == 18 and precision != "fp16":  # (the 4-phase ConvTranspose case runs in fp16 only)
            continue
        sd = _model(C)
        img = LR.case_frames(h, w, B)[1].double()
        stored = LR.emulated_forward(sd, LR.HEIGHTS, LR.DOWNSAMPLES, img, precision)
        rep = LR.check(sd, LR.HEIGHTS, LR.DOWNSAMPLES, img, precision, stored)
        assert len(rep.rows) == 46 and not rep.skipped
        d, s = rep.worst()
        print(f"C={C} {h}x{w} B={B} {precision}: {d:.3f} x deterministic, {s:.3f} x u(|ref|+Q)")
        assert not rep.failures(LR.C_STAT[precision]), rep.failures(LR.C_STAT[precision])
        worst_det, worst_stat = max(worst_det, d), max(worst_stat, s)
    record_measurement(f"layers/cpu/{precision}", {"max_det_ratio": worst_det, "c_measured": worst_stat})
    # C_MEASURED is this number (fp32 summation order of the host's convolution may move it a little)
    assert abs(worst_stat - LR.C_MEASURED[precision]) <= 0.05 * LR.C_MEASURED[precision], worst_stat


# ---- one layer at a time: the 100x140 case at B = 1 ----
S1 = "backbone.multi_ida_up.ida_up_layers.0.output_layers.0.0"       # 3x3 s1, 25x35
S2 = "backbone.dla_down.block_layers.1.conv1"                        # 3x3 s2, 50x70 -> 25x35
RES = "backbone.dla_down.block_layers.1.conv2+conv_residual"         # 3x3 s1 (25x35) + 1x1 s2 (50x70)
ROOT = "backbone.dla_down.tree_layers.0.root.conv"                   # 1x1 over [left, right], 13x18
CONVT = "backbone.ida_up_reverse.upsample_layers.1+pad_to_match+add"  # s = 4: 7x9 -> 28x36 -> 25x35
TILE_W, TILE_H = 32, 16


@functools.lru_cache(maxsize=None)
def _g1(precision):
    sd = _model(128)
    img = LR.case_frames(100, 140, 1)[1].double()
    vals = LR.emulated_forward(sd, LR.HEIGHTS, LR.DOWNSAMPLES, img, precision)
    return LR.layer_graph(sd, LR.HEIGHTS, LR.DOWNSAMPLES), vals


def _judge(layer, xs, got, precision, r=1):
    ref = LR.evaluate(layer, xs)
    det, stat = LR.bounds(layer, xs, ref, precision, r)
    return LR.ratios(got, ref, det, stat)


def _assert_fault(layer, xs, good, bad, touched, precision, r=1):
    """`bad` differs from `good` only where `touched`; good passes, bad breaks both bounds there."""
    c = LR.C_STAT[precision]
    rd, rs = _judge(layer, xs, good, precision, r)
    assert float(rd.max()) <= 1.0 and float(rs.max()) <= c, (float(rd.max()), float(rs.max()))
    assert torch.equal(bad[~touched], good[~touched])
    rd, rs = _judge(layer, xs, bad, precision, r)
    assert float(rd[touched].max()) > 1.0, float(rd[touched].max())
    assert float(rs[touched].max()) > c, float(rs[touched].max())
    if bool((~touched).any()):  # (a 13-row map is one partial tile row: everything is touched)
        assert float(rd[~touched].max()) <= 1.0 and float(rs[~touched].max()) <= c
    return float(rd[touched].max()), float(rs[touched].max())


def _halo_fault(layer, xs, precision):
    """Output column TILE_W - 1 computed with its right halo column (segment 0's input) as zero."""
    src, w, stride, pad = layer.segs[0]
    ox = TILE_W - 1
    x0 = ox * stride + 1
    assert x0 < xs[src].shape[3]
    broken = LR.Layer(layer.label, layer.kind, [("halo", w, stride, pad)] + layer.segs[1:], layer.bias, layer.act,
                      layer.skip, layer.out_f32, layer.K)
    xs2 = dict(xs)
    xs2["halo"] = xs[src].clone()
    xs2["halo"][..., x0] = 0
    good = LR.emulate(layer, xs, precision)
    bad = good.clone()
    bad[..., ox] = LR.emulate(broken, xs2, precision)[..., ox]
    touched = torch.zeros_like(good, dtype=torch.bool)
    touched[..., ox] = True
    return good, bad, touched


def _kstep_fault(layer, xs, precision):
    """The last (partial) tile row computed without input channels 32..63 of one tap of segment 0."""
    kh = layer.segs[0][1].shape[2]
    tap = (1, 2) if kh == 3 else (0, 0)

    def drop(i, w):
        if i == 0:
            w = w.clone()
            w[:, 32:64, tap[0], tap[1]] = 0
        return w
    good = LR.emulate(layer, xs, precision)
    y0 = (good.shape[2] - 1) // TILE_H * TILE_H
    assert good.shape[2] % TILE_H, "the last tile row is to be a partial one"
    bad = good.clone()
    bad[:, :, y0:] = LR.emulate(layer, xs, precision, weight_fault=drop)[:, :, y0:]
    touched = torch.zeros_like(good, dtype=torch.bool)
    touched[:, :, y0:] = True
    return good, bad, touched


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("label", [S1, S2, RES])
def test_halo_column_read_as_zero_breaks_the_bounds(label, precision):
    layers, vals = _g1(precision)
    layer = layers[label]
    xs = {s: vals[s] for s in layer.sources()}
    rd, rs = _assert_fault(layer, xs, *_halo_fault(layer, xs, precision), precision)
    print(f"{label} {precision}: {rd:.3g} x deterministic, {rs:.3g} x u(|ref|+Q)")


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("label", [S1, S2, RES, ROOT])
def test_dropped_k_step_breaks_the_bounds(label, precision):
    layers, vals = _g1(precision)
    layer = layers[label]
    xs = {s: vals[s] for s in layer.sources()}
    rd, rs = _assert_fault(layer, xs, *_kstep_fault(layer, xs, precision), precision)
    print(f"{label} {precision}: {rd:.3g} x deterministic, {rs:.3g} x u(|ref|+Q)")


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_convt_target_one_column_off_breaks_the_bounds(precision):
    layers, vals = _g1(precision)
    layer = layers[CONVT]
    xs = {s: vals[s] for s in layer.sources()}
    src, w, s, _ = layer.segs[0]
    skip = xs[layer.skip]
    assert (xs[src].shape[2] * s, xs[src].shape[3] * s) == (28, 36) and tuple(skip.shape[2:]) == (25, 35)
    # the shift: F.pad's tuple quirk pads W by the H excess (one zero column on the left), then the crop
    z = torch.ones((1, 1, 28, 36), dtype=torch.float64)
    assert float(pad_to_match(z, skip.shape)[0, 0, :, 0].abs().max()) == 0.0
    dt = LR.TORCH_DTYPE[precision]
    wr = w.float().to(dt).float()
    u = pad_to_match(F.conv_transpose2d(xs[src].float(), wr, layer.bias.float(), stride=s), skip.shape)
    good = (u + skip.float()).to(dt).double()
    assert torch.equal(good, LR.emulate(layer, xs, precision))
    off = torch.zeros_like(u)
    off[..., 1:] = u[..., :-1]
    bad = (off + skip.float()).to(dt).double()
    c = LR.C_STAT[precision]
    rd, rs = _judge(layer, xs, good, precision)
    assert float(rd.max()) <= 1.0 and float(rs.max()) <= c
    rd, rs = _judge(layer, xs, bad, precision)
    # every column is written from its neighbour's values and holds elements past both bounds (but
    # column 0: the margin the shift left uncovered stays the skip tensor either way)
    assert bool((rd.amax((0, 1, 2))[1:] > 1.0).all()) and bool((rs.amax((0, 1, 2))[1:] > c).all())
    assert torch.equal(bad[..., 0], good[..., 0])


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("fault", [_halo_fault, _kstep_fault])
def test_fused_heads_chain(fault, precision):
    """The hidden layer is not stored when the 1x1 heads run in the 3x3 heads' epilogue (which keeps
    it at ~fp32: a hi + lo pair): the head output is judged over the chain with r = 1, and a fault in
    the hidden 3x3 still breaks the bounds."""
    layers, vals = _g1(precision)
    hid, out = layers[HEADS_HIDDEN_LABEL], layers[HEADS_OUT_LABEL]
    xs = {s: vals[s] for s in hid.sources()}
    hid = LR.Layer(hid.label, hid.kind, hid.segs, hid.bias, hid.act, None, True, hid.K)  # (fp32, not rounded)
    good_h, bad_h, touched_h = fault(hid, xs, precision)
    chain = {HEADS_HIDDEN_LABEL: LR.evaluate(hid, xs)}  # what the oracle passes through
    good = LR.emulate(out, {HEADS_HIDDEN_LABEL: good_h}, precision)
    bad = LR.emulate(out, {HEADS_HIDDEN_LABEL: bad_h}, precision)
    touched = touched_h[:, :good.shape[1]]  # the 1x1 keeps the pixel: the same rows / column of every output channel
    rd, rs = _assert_fault(out, chain, good, bad, touched, precision, r=1)
    print(f"fused heads {fault.__name__} {precision}: {rd:.3g} x deterministic, {rs:.3g} x u(|ref|+Q)")


def test_oracle_hook_is_transparent():
    """hook=None is the default path; an identity hook sees every engine op once, in order, and
    changes nothing."""
    import oracle
    sd = _model(64)
    img = LR.case_frames(36, 44, 1)[1].double()
    seen = []
    with torch.no_grad():
        a = oracle.centernet_forward(sd, img, LR.HEIGHTS, LR.DOWNSAMPLES, dict(keypoints=False))
        b = oracle.centernet_forward(sd, img, LR.HEIGHTS, LR.DOWNSAMPLES, dict(keypoints=False),
                                     hook=lambda label, t: (seen.append(label), t)[1])
    assert seen == list(LR.layer_graph(sd, LR.HEIGHTS, LR.DOWNSAMPLES))
    for f in ("heatmap", "size", "offset"):
        assert torch.equal(getattr(a, f), getattr(b, f))
