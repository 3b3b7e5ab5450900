"""Every op of the native YOLACT plans on its own, at odd sizes, against float64, on the routes the
B = 32 benchmark takes (TV_ARCH_RESNET18, TV_ARCH_YOLACT_HEAD, TV_ARCH_YOLACT).

tests/yolact_layer_ref.py has the graph, the bounds and their derivation per op kind;
tests/test_yolact_layer_ref_cpu.py shows on the CPU that the graph is the float64 restatements, that
seven injected faults (a stride-2 residual read at stride 1, a BatchNorm scale left out of an identity
segment, a residual dropped on a partial tile row, an unclamped bilinear tap, swapped ConvTranspose
phases, ratio-major head rows, a dropped last k-step at 512 channels) break both bounds, and measures
the statistical constant: c_measured = 1.92 (fp16) / 2.03 (bf16), asserted here at twice that
(yolact_layer_ref.C_STAT_YOLACT = 3.84 / 4.06). fp32 is judged by the deterministic bound
K 2^-24 A + 2^-24 |ref| alone (its statistical ratio is recorded).

Backbone (Resnet101Backbone, seeded weights, a normal fp32 NCHW image): the smallest geometries with
a full and a partial conv3x3 tile (32x16 / 16x32 pixels at 8 waves) where the route allows one:
  R1 200x280 B=3  conv1 100x140, pool / layer1 50x70, layer2 25x35, layer3 13x18, layer4 7x9: partial
                  tiles both ways at 64 and 128 channels, stride-2 inputs of both parities
  R2 149x77  B=1  conv1 75x39 (odd both ways: the fused stem's out-of-map conv row / column), 38x20,
                  19x10, 10x5, 5x3: width under one 32-wide tile
  R3 37x51   B=5  every map inside one tile, B h w no multiple of 32, 2x2 deepest map
Head (YolactHead, depths (128, 256, 512), C = 7, k = 8, layers (1, 0, 0, 0), two extra levels):
  H1 F=256 ars (1, 2) maps 13x18 / 7x9 / 4x5 B=3: bilinear 7->13, 9->18, 4->7, 5->9; protonet up to
                  52x72 (convt3 on 13x18 and 26x36); head blocks at 64 channels; final conv N = 40
  H2 F=256 ars (1,)  maps 25x35 / 13x18 / 7x9 B=1: partial tiles on the FPN and head layers; N = 20
  H3 F=128 ars (1,)  maps as H1 B=3: the FPN stride-2 layers on conv3x3s2 (TV_S2_MINTILES=0), the
                  32-channel Bottleneck on conv_small
Whole model (Yolact): R2's image, H1's head fields, B=2: the taps feed the laterals from the arena.
No map was shrunk and no batch lowered to keep the time: the slowest case is below.

Legs: test_gpu_layers.LEGS (engine._DIAG_KNOBS) and the YOLACT knobs on top of its halo leg; each
asserts from the kernel names that the family under test ran before anything is compared
(_assert_backbone_family, _assert_head_family). Each case also asserts that the tap changes nothing:
the caller's outputs of op_outputs_multi equal forward_multi's bit for bit.

Measured on MI355X, zero failing layers on every leg (largest ratio over the layers of each leg:
x deterministic bound / x u(|ref|+Q), then the same over the matrix ops alone — conv and convt3 rows:
the rounding-only ops (staging, layout, add_relu) reach ~1.0 x their bound by construction, a value
that rounds by half an ulp; recorded per case under "yolact_layers/..." by helpers.record_measurement):
  default              fp16  0.999 / 1.948   0.827 / 1.948   R1 B3, R2 B1, R3 B5, H1 B3, H2 B1, H3 B3, W B2
  default              bf16  0.996 / 2.030   0.854 / 2.030   R1 B3, R2 B1, R3 B5, H1 B3, H2 B1, H3 B3, W B2
  default              fp32  0.500 / (170)   0.019 / (45.8)  R2 B1, H1 B3   (statistical ratio not asserted)
  halo                 fp16  0.999 / 1.917   0.822 / 1.917   R1 B3, R2 B1, R3 B5, H1 B3, H2 B1, H3 B3, W B2
  halo                 bf16  0.996 / 2.030   0.854 / 2.030   R1 B3, R2 B1, R3 B5, H1 B3, H2 B1, H3 B3, W B2
  cus8                 fp16  0.999 / 1.917   0.822 / 1.917   R1 B3, R2 B1, R3 B5, H1 B3, H2 B1, H3 B3
  cus8                 bf16  0.996 / 2.030   0.854 / 2.030   R1 B3, R2 B1, R3 B5, H1 B3, H2 B1, H3 B3
  cus8+TV_C3_NI=4      fp16  0.999 / 1.677   0.378 / 1.677   R1 B3
  cus8+TV_C3_TW=16     fp16  0.999 / 1.677   0.378 / 1.677   R1 B3
  cus8+TV_C3_TW=32     fp16  0.999 / 1.677   0.378 / 1.677   R1 B3
  halo+TV_RSTEM=0      fp16  0.999 / 1.696   0.382 / 1.696   R1 B3
  halo+TV_CT3=0        fp16  0.999 / 1.794   0.739 / 1.794   H1 B3
  halo+TV_C1X1=0       fp16  0.999 / 1.794   0.739 / 1.794   H1 B3   (the backbone has no stride-1 1x1 conv)
  generic              fp16  0.999 / 1.913   0.739 / 1.913   R1 B3, H1 B3
  lat                  fp16  0.999 / 1.777   0.739 / 1.777   R1 B3, H1 B3
  burst                fp16  0.999 / 1.792   0.749 / 1.792   R1 B3, H1 B3
The matrix ops' largest deterministic ratios (0.7-0.85) are the head block's last GEMM: its BatchNorm-scaled
identity term dominates A, so the error is the rounding of one scale, which the bound meets closely.
Device tanhf against float64 tanh of the stored raw value: at most 8.4e-8 (bar 1e-4).
Slowest case: the whole model, 0.6-0.8 s (the existing suite's slowest layer case: 8.2 s); every other case at most 0.5 s.
The halo / cus8 kernel lists of R1 are DESIGN §10's route table, B = 32 column, row by row (stem7s2_pool;
layer1 conv3x3 on 64-channel half tiles, RES on conv2; the three stride-2 convs and layer4 on conv_pipe;
layerL.0.conv2 + downsample on conv3x3 RES; layerL.1 on conv3x3; add_relu); the table does not say that
layer2.1 runs the 4-wave conv3x3 instance (NW = 4) at these sizes. H2's head ops have no table in §10:
their routes are what _assert_head_family states (laterals and the blocks' 1x1 GEMMs on conv1x1_stream,
FPN / protonet 3x3 on conv3x3, stride-2 FPN convs on conv_pipe, convt3, `_layers_3` with the fused 1x1
epilogue, final convs on conv_pipe with the fp32 store), and tests/data/kernel_routes.json pins the head
archs' tables at the benchmark geometry.
The recorded files: profiles/layers/yolact_layers_gpu.json (this table's cases), profiles/layers/layers_cpu.json (c).
"""
import time

import pytest
import torch

import layer_ref as LR
import test_gpu_layers as TL
import yolact_layer_ref as YL
from helpers import record_measurement

pytestmark = pytest.mark.gpu

HALO, CUS8 = TL.HALO, TL.CUS8
LEGS = dict(TL.LEGS)
LEGS["generic"] = dict(TL.LEGS["generic"], TV_CT3="0", TV_RSTEM="0")  # (the YOLACT plans' hand-written kernels too)
for _k in ("TV_RSTEM", "TV_CT3", "TV_C1X1"):
    LEGS[f"halo+{_k}=0"] = dict(HALO, **{_k: "0"})
HAND_WRITTEN = TL.HAND_WRITTEN + ("tv::ct3::", "tv::csm::", "tv::rn::stem7s2_pool<")
C3, PIPE, IGEMM = "tv::c3::conv3x3<", "tv::pipe::conv_pipe<", "tv::conv_igemm<"
GEMM_T = {"fp16": "_Float16", "bf16": "__bf16", "fp32": "float"}


def _targs(kernel):
    return kernel.split("<", 1)[1].rstrip(">").split(", ")


def _halo_like(leg):
    return leg.startswith(("halo", "cus8"))


def _assert_backbone_family(leg, precision, kern, layers, pre=""):
    """The ResNet ops of the leg's family really run it (a leg cannot pass vacuously)."""
    knobs = LEGS[leg]
    convs = [k for k, l in layers.items() if l.kind == "conv" and k.startswith(pre + "layer")]
    stem, pool = pre + "conv1 + bn1 + ReLU", pre + "maxpool"
    fused = precision != "fp32" and knobs.get("TV_RSTEM") != "0"
    assert kern[pool].startswith("tv::rn::stem7s2_pool<" if fused else "tv::rn::maxpool3x3s2<"), kern[pool]
    assert kern[stem].startswith("(fused into the max-pool" if fused else (PIPE, IGEMM)), kern[stem]
    assert kern[YL.STAGE] == ("prep (fused into the stem)" if fused else "prep"), kern[YL.STAGE]
    for k, l in layers.items():
        if l.kind == "add_relu":
            assert kern[k].startswith("tv::rn::add_relu<"), (k, kern[k])
        if l.kind == "store_f32":
            assert kern[k].startswith("tv::rn::store_f32<"), (k, kern[k])
    if leg == "generic" or precision == "fp32":
        bad = {k: kern[k] for k in convs if not kern[k].startswith((PIPE, IGEMM, "tv::lat::conv_lat<"))}
        assert not bad and (precision == "fp32" or not any(v.startswith("tv::lat::") for v in kern.values())), bad
    elif leg == "lat":
        not_lat = {k: kern[k] for k in convs if not kern[k].startswith("tv::lat::conv_lat<")}
        assert not not_lat, not_lat
    elif leg == "burst":
        # what conv_burst represents here: a 3x3 / stride 1 window over a 128-channel multiple with K <= 1280
        for k in (pre + "layer2.1.conv1 + bn1 + ReLU", pre + "layer2.1.conv2 + bn2 (tap)"):
            assert kern[k].startswith("tv::burst::conv_burst<"), (k, kern[k])
    elif _halo_like(leg):  # DESIGN §10's route table, B = 32 column
        for k in convs:
            L, blk = int(k[len(pre) + 5]), int(k[len(pre) + 7])
            s2 = blk == 0 and L > 1 and ".conv1" in k
            if L == 4 or s2:
                assert kern[k].startswith(PIPE), (k, kern[k])
                continue
            assert kern[k].startswith(C3), (k, kern[k])
            a = _targs(kern[k])
            res = ".conv2 + bn2 + x" in k or "downsample" in k
            assert a[5] == ("1" if res else "0"), (k, kern[k])
            assert a[7] == str(layers[k].segs[0][1].shape[1] // 32), (k, kern[k])
            if L == 1:
                assert a[6] == "2", (k, kern[k])  # one 64-channel half tile holds every output channel
            if "TV_C3_TW" in knobs:
                assert a[2] == knobs["TV_C3_TW"], (k, kern[k])
            if "TV_C3_NI" in knobs and L > 1:
                assert a[6] == knobs["TV_C3_NI"], (k, kern[k])


def _assert_head_family(leg, precision, kern, layers, F):
    """The neck, protonet and head ops of the leg's family really run it."""
    knobs = LEGS[leg]
    lat = [k for k in layers if "_lateral_layers." in k]
    pred = [k for k in layers if "_prediction_layers." in k]
    down = [k for k in layers if "_downsample_layers." in k]
    proto3 = [k for k in layers if k.startswith(YL.MN + "_layers_")]
    ups = [k for k, l in layers.items() if l.kind == "convt3"]
    phases = [k for k, l in layers.items() if l.kind == "phase"]
    finals = [k for k in layers if "final 3x3 convs" in k]
    conv2 = [k for k in layers if k.endswith("_extra_layers.0.conv2")]
    one = [k for k in layers if k.endswith(("_extra_layers.0.conv1", "_extra_layers.0.conv3 + x", "(bottleneck)"))]
    out = YL.MN + "_output_layer + LeakyReLU -> fp32 NHWC"
    for k, l in layers.items():
        if l.kind == "bilinear_add":
            assert kern[k].startswith("tv::yh::bilinear_add<"), (k, kern[k])
        if l.kind == "head_scatter":
            assert kern[k] == "tv::yh::head_scatter", (k, kern[k])
        if l.kind == "layout_in":
            assert kern[k].startswith("tv::nchw_to_nhwc<"), (k, kern[k])
    f32out = f"<{GEMM_T[precision]}, float, 0"
    for k in finals:  # a generic GEMM with the fp32 store, on every leg
        assert kern[k].startswith((PIPE, IGEMM)) and f32out in kern[k], (k, kern[k])
    if leg == "generic" or precision == "fp32":
        bad = {k: v for k, v in kern.items() if v.startswith(HAND_WRITTEN) and not v.startswith("tv::lat::")}
        assert not bad, bad
        assert all(kern[k].startswith((PIPE, IGEMM)) for k in ups + phases), [kern[k] for k in ups + phases]
        assert kern[out].startswith((PIPE, IGEMM)), kern[out]
    elif leg == "lat":
        n = sum(v.startswith("tv::lat::conv_lat<") for v in kern.values())
        assert n >= len(lat) + len(pred) + len(down) + len(conv2) + len(one), (n, kern)
    elif leg == "burst":
        assert sum(v.startswith("tv::burst::conv_burst<") for v in kern.values()) >= len(lat), kern
    elif _halo_like(leg):
        for k in pred + proto3:
            assert kern[k].startswith(C3) and _targs(kern[k])[7] == str(F // 32), (k, kern[k])
        fused = _targs(kern[proto3[-1]])[4] == "1" and kern[out] == "(fused into the 3x3 heads)"
        assert fused, (kern[proto3[-1]], kern[out])
        for k in down:
            assert kern[k].startswith("tv::c3s2::conv3x3s2<" if F == 128 else PIPE), (k, kern[k])
        for k in conv2:
            assert kern[k].startswith("tv::csm::conv_small" if F == 128 else C3), (k, kern[k])
        if knobs.get("TV_CT3") == "0":
            gemms = [kern[k] for k in ups + phases]  # each phase a GEMM with the phase-scatter epilogue (MODE 1)
            assert all(v.startswith(PIPE) and _targs(v)[2].startswith("1") for v in gemms), gemms
        else:
            assert all(kern[k].startswith("tv::ct3::convt3<") for k in ups), [kern[k] for k in ups]
            assert all(kern[k].startswith("(fused into the phase (0,0)") for k in phases), [kern[k] for k in phases]
        c1 = "tv::c1x1::conv1x1_stream<"
        for k in lat + one:
            assert kern[k].startswith((PIPE,) if knobs.get("TV_C1X1") == "0" else (c1, PIPE)), (k, kern[k])
        if knobs.get("TV_C1X1") != "0":
            assert any(kern[k].startswith(c1) for k in lat + one), [kern[k] for k in lat + one]


def _finish(key, t0, rep, precision, kern, layers):
    det, stat = rep.worst()
    # (the rounding-only ops sit at ~1.0 x their bound by construction: the matrix ops on their own too)
    mm = [r for r in rep.rows if layers[r[0]].kind in ("conv", "convt3")]
    mm_det, mm_stat = max(r[3] for r in mm), max(r[4] for r in mm)
    took = time.time() - t0
    fams = {}
    for v in kern.values():
        f = v.split("<", 1)[0]
        fams[f] = fams.get(f, 0) + 1
    c = YL.C_STAT_YOLACT.get(precision)
    record_measurement(key, {"det_ratio": det, "stat_ratio": stat, "conv_det_ratio": mm_det, "conv_stat_ratio": mm_stat,
                             "c": c, "tanh_err": rep.tanh_err,
                             "not_stored": [k for k in rep.skipped if " phase (" not in k], "kernels": fams,
                             "seconds": took})
    print(f"{key}: {det:.3f} x deterministic, {stat:.3f} x u(|ref|+Q) (c = {c}; convs {mm_det:.3f} / {mm_stat:.3f}), "
          f"{len(rep.rows)} layers compared, "
          f"{len(rep.skipped)} not stored, tanh {rep.tanh_err:.2e}, {took:.1f} s")
    fails = rep.failures(c if c is not None else float("inf"))
    assert not fails, "\n".join(fails)


def _stored(rows):
    kern = {label: k for label, k, _ in rows}
    return kern, {label: (None if t is None else LR.nchw64(t)) for label, _, t in rows}


def _tap_backbone(geometry, precision, B=None):
    from tauv_vision_amd.yolact import Resnet101Backbone
    sd, sd64, img = YL.backbone_case(geometry, B)
    bb = Resnet101Backbone(None, precision=precision)
    bb.load_state_dict({"_feature_extractor." + k: v for k, v in sd.items()}, strict=True)
    x = img.cuda()
    taps = bb.forward_nhwc(x)
    eng = next(iter(bb._engines.values()))
    outs = [torch.empty_like(t) for t in taps]
    rows = eng.op_outputs_multi([x], outs)
    torch.cuda.synchronize()
    for a, b in zip(outs, taps):  # the tap (one op per launch) changes nothing
        assert torch.equal(a, b)
    return sd64, img, rows


def _run_backbone(monkeypatch, leg, geometry, precision):
    from tauv_vision_amd import engine as E
    t0 = time.time()
    monkeypatch.setattr(E, "_DIAG_KNOBS", dict(LEGS[leg]))
    sd64, img, rows = _tap_backbone(geometry, precision)
    kern, stored = _stored(rows)
    layers, _ = YL.resnet18_layers(sd64)
    for label in layers:
        assert kern.get(label), (label, kern)
    _assert_backbone_family(leg, precision, kern, layers)
    with torch.no_grad():
        rep = YL.check(layers, {YL.IMG: img.double()}, precision, stored, kern)
    _finish(f"yolact_layers/resnet18/{leg}/{geometry}/B{img.shape[0]}/{precision}", t0, rep, precision, kern, layers)


def _tap_head(geometry, precision, extra=None):
    from tauv_vision_amd.yolact import YolactHead
    c, sd, sd64, maps = YL.head_case(geometry)
    head = YolactHead(c["depths"], YL.head_config(c), precision=precision)
    head.load_state_dict(sd)
    xs = [m.cuda() for m in maps]
    want = head(xs)
    eng = head.engine(xs[0].device, tuple(c["sizes"]))
    h, w = c["sizes"][0]
    outs = [torch.empty_like(want[0]), torch.empty_like(want[1]), torch.empty_like(want[2]),
            torch.empty((c["batch"], 4 * h, 4 * w, (c["k"] + 3) // 4 * 4), device=xs[0].device)]
    rows = eng.op_outputs_multi(xs, outs)
    torch.cuda.synchronize()
    for a, b in zip(outs[:3], want[:3]):
        assert torch.equal(a, b)
    assert torch.equal(outs[3][..., :c["k"]].permute(0, 3, 1, 2), want[4])
    return c, sd64, maps, rows, tuple(o.double().cpu() for o in outs[:3])


def _run_head(monkeypatch, leg, geometry, precision):
    from tauv_vision_amd import engine as E
    t0 = time.time()
    knobs = dict(LEGS[leg])
    if geometry == "H3" and _halo_like(leg):
        knobs["TV_S2_MINTILES"] = "0"
    monkeypatch.setattr(E, "_DIAG_KNOBS", knobs)
    c, sd64, maps, rows, heads = _tap_head(geometry, precision)
    kern, stored = _stored(rows)
    layers, _, _ = YL.yolact_head_layers(sd64, 3, c["down"], c["layers"], len(c["ars"]))
    for label in layers:
        assert kern.get(label), (label, kern)
    _assert_head_family(leg, precision, kern, layers, c["F"])
    with torch.no_grad():
        rep = YL.check(layers, {f"map{i}": m.double() for i, m in enumerate(maps)}, precision, stored, kern, heads)
    _finish(f"yolact_layers/head/{leg}/{geometry}/B{c['batch']}/{precision}", t0, rep, precision, kern, layers)


def _run_whole(monkeypatch, leg, precision):
    from tauv_vision_amd import engine as E
    from tauv_vision_amd.yolact import Resnet101Backbone, Yolact
    t0 = time.time()
    monkeypatch.setattr(E, "_DIAG_KNOBS", dict(LEGS[leg]))
    c, sd, sd64, img = YL.whole_case()
    cfg = YL.head_config(c)
    net = Yolact(cfg, backbone=Resnet101Backbone(cfg, precision), precision=precision)
    net.load_state_dict(sd, strict=True)
    x = img.cuda()
    want = net(x)
    eng = next(iter(net._engines.values()))
    outs = [torch.empty_like(want[0]), torch.empty_like(want[1]), torch.empty_like(want[2]),
            torch.empty((c["batch"], want[4].shape[2], want[4].shape[3], (c["k"] + 3) // 4 * 4), device=x.device)]
    rows = eng.op_outputs_multi([x], outs)
    torch.cuda.synchronize()
    for a, b in zip(outs[:3], want[:3]):
        assert torch.equal(a, b)
    assert torch.equal(outs[3][..., :c["k"]].permute(0, 3, 1, 2), want[4])
    kern, stored = _stored(rows)
    layers, _, _ = YL.yolact_layers(sd64, c["down"], c["layers"], len(c["ars"]))
    for label in layers:
        assert kern.get(label), (label, kern)
    _assert_backbone_family(leg, precision, kern, layers, YL.BB)
    _assert_head_family(leg, precision, kern, layers, c["F"])
    # the taps feed the laterals from the arena: no layout op, no fp32 store
    assert not any(l.kind in ("layout_in", "store_f32") for l in layers.values())
    with torch.no_grad():
        heads = tuple(o.double().cpu() for o in outs[:3])
        rep = YL.check(layers, {YL.IMG: img.double()}, precision, stored, kern, heads)
    _finish(f"yolact_layers/yolact/{leg}/W/B{c['batch']}/{precision}", t0, rep, precision, kern, layers)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("geometry", ["R1", "R2", "R3"])
@pytest.mark.parametrize("leg", ["default", "halo", "cus8"])
def test_backbone_layers(monkeypatch, leg, geometry, precision):
    _run_backbone(monkeypatch, leg, geometry, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("geometry", ["H1", "H2", "H3"])
@pytest.mark.parametrize("leg", ["default", "halo", "cus8"])
def test_head_layers(monkeypatch, leg, geometry, precision):
    _run_head(monkeypatch, leg, geometry, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("leg", ["default", "halo"])
def test_whole_model_layers(monkeypatch, leg, precision):
    _run_whole(monkeypatch, leg, precision)


@pytest.mark.parametrize("leg", ["cus8+TV_C3_NI=4", "cus8+TV_C3_TW=16", "cus8+TV_C3_TW=32", "halo+TV_RSTEM=0",
                                 "generic", "lat", "burst"])
def test_backbone_kernel_variants(monkeypatch, leg):
    _run_backbone(monkeypatch, leg, "R1", "fp16")


@pytest.mark.parametrize("leg", ["halo+TV_CT3=0", "halo+TV_C1X1=0", "generic", "lat", "burst"])
def test_head_kernel_variants(monkeypatch, leg):
    _run_head(monkeypatch, leg, "H1", "fp16")


def test_backbone_layers_fp32(monkeypatch):
    """The fp32 plan: the stem unfused by construction, store_f32 exact (bound 0)."""
    _run_backbone(monkeypatch, "default", "R2", "fp32")


def test_head_layers_fp32(monkeypatch):
    _run_head(monkeypatch, "default", "H1", "fp32")
