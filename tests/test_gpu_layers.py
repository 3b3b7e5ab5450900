"""Every layer of the native CenterNet forward on its own, at odd sizes, against float64.

tests/layer_ref.py has the method (teacher-forced per-layer comparison, the two bounds and their
derivation); tests/test_layer_ref_cpu.py shows on the CPU that it fails for a zeroed halo column,
a dropped k-step on a partial tile row and a ConvTranspose target one column off, and measures the
statistical constant: c_measured = 1.96 (fp16) / 2.31 (bf16), asserted here at twice that
(layer_ref.C_STAT = 3.92 / 4.62).

Model: tv.Centernet(tv.DLABackbone([1, 1, 1], [C] * 4, 2), 4 plain labels), heads [4, 2, 2], seeded
weights; C = 128, and C = 64 for the two-channel-block conv3x3 body. Geometries (the smallest with a
full and a partial tile):
  G1 100x140 B=3  maps 50x70, 25x35, 13x18, 7x9, 4x5: partial tiles both ways, crops 26 -> 25 and
                  36 -> 35, the s = 4 step 28x36 -> 25x35 with the H-excess-pads-W shift
  G2 148x76  B=1  maps 74x38 ... 5x3: width under one 32-wide tile, 16x32 tiles with 27 rows outside
  G3 36x44   B=5  every map inside one tile, B*h*w no multiple of 32: convt tiles straddle frames
Legs (engine._DIAG_KNOBS, as tests/test_gpu_conv_lat.py): LEGS below; each asserts from the kernel
names that its ops run the family under test before anything is compared. Each case also runs the
normal model forward (grouped launches) against the un-hooked float64 oracle under
test_gpu_forward.TOL.

Measured on MI355X (largest ratio over the layers of each leg: x deterministic bound / x u(|ref|+Q);
recorded per case under "layers/..." by helpers.record_measurement):
  default              fp16  0.507 / 3.298   G1 B3, G2 B1, G3 B5
  default              bf16  0.497 / 3.560   G1 B3, G2 B1, G3 B5
  halo                 fp16  0.479 / 3.298   G1 B3, G1 B3 u8, G2 B1, G3 B5
  halo                 bf16  0.513 / 3.560   G1 B3, G1 B3 u8, G2 B1, G3 B5
  cus8                 fp16  0.544 / 3.624   G1 B18, G1 B3
  cus8                 bf16  0.513 / 3.560   G1 B3
  cus8 C=64            fp16  0.595 / 2.601   G1 B3
  cus8 C=64            bf16  0.644 / 2.606   G1 B3
  cus8+TV_C3_TW=16     fp16  0.477 / 3.251   G1 B3
  cus8+TV_C3_TW=32     fp16  0.458 / 3.251   G1 B3
  cus8+TV_C3_NI=2      fp16  0.458 / 3.251   G1 B3
  cus8+TV_C3_NI=4      fp16  0.519 / 3.251   G1 B3
  cus8+TV_C3_NW=8      fp16  0.458 / 3.251   G1 B3
  cus8+TV_STEMFUSE=0   fp16  0.484 / 2.568   G1 B3
  cus8+TV_HEADFUSE=0   fp16  0.458 / 3.251   G1 B3
  lat                  fp16  0.514 / 3.298   G1 B3, G3 B5
  burst                fp16  0.507 / 3.298   G1 B3, G3 B5
  generic              fp16  0.486 / 2.657   G1 B3, G3 B5
Slowest case: cus8/C128/G1/B18/fp16 8.2 s (its float64 oracle runs over 18 frames); every other case at most 2.3 s.
The recorded files: profiles/layers/layers_gpu.json (this table's cases), profiles/layers/layers_cpu.json (c).
"""
import functools
import time

import pytest
import torch

import layer_ref as LR
import oracle
import test_gpu_forward as fwd
from helpers import record_measurement
from oracle.ref_forward import HEADS_HIDDEN_LABEL, HEADS_OUT_LABEL

pytestmark = pytest.mark.gpu

GEOMETRIES = {"G1": (100, 140, 3), "G2": (148, 76, 1), "G3": (36, 44, 5)}
B_4PHASE = 18  # G1 on 8 CUs: convt_schedule groups 4 phases of the 13x18 -> 25x35 steps from this batch on
                # (test_layers_convt_four_phase_groups asserts both that and that 17 does not)
HALO = {"TV_LAT": "0", "TV_BURST": "0"}
CUS8 = dict(HALO, TV_CUS="8")
LEGS = {
    "default": {},
    "halo": HALO,
    "cus8": CUS8,
    "lat": {"TV_LAT_UNITS": str(10 ** 9), "TV_BURST": "0"},
    "burst": {"TV_BURST": "2"},
    "generic": {"TV_CONV3": "0", "TV_CONV3S2": "0", "TV_CONVT": "0", "TV_STEM": "0", "TV_LAT": "0", "TV_BURST": "0",
                "TV_C1X1": "0"},
}
for _k, _v in (("TV_C3_TW", "16"), ("TV_C3_TW", "32"), ("TV_C3_NI", "2"), ("TV_C3_NI", "4"), ("TV_C3_NW", "8"),
               ("TV_STEMFUSE", "0"), ("TV_HEADFUSE", "0")):
    LEGS[f"cus8+{_k}={_v}"] = dict(CUS8, **{_k: _v})

STEM = LR.STEM
BLOCK0_CONV1 = "backbone.dla_down.block_layers.0.conv1"
UP_S2 = "backbone.ida_up_reverse.upsample_layers.0+pad_to_match+add"  # s = 2: 13x18 -> 26x36 -> 25x35
UP_S4 = "backbone.ida_up_reverse.upsample_layers.1+pad_to_match+add"  # s = 4: 7x9 -> 28x36 -> 25x35
HAND_WRITTEN = ("tv::c3::", "tv::c3s2::", "tv::convt::", "tv::stem::", "tv::ss2::", "tv::lat::", "tv::burst::",
                "tv::c1x1::")


@functools.lru_cache(maxsize=None)
def _weights(C):
    return LR.make_model(C, "fp16")[1]


@functools.lru_cache(maxsize=None)
def _oracle(C, h, w, B):
    """The un-hooked float64 oracle of a case: computed once, shared by every leg."""
    img = LR.case_frames(h, w, B)[1].double()
    with torch.no_grad():
        p = oracle.centernet_forward(_weights(C), img, LR.HEIGHTS, LR.DOWNSAMPLES, dict(keypoints=False))
    return {f: getattr(p, f) for f in ("heatmap", "size", "offset")}


def _lib_label(eng, i):
    from tauv_vision_amd import _lib
    return _lib.lib().tv_engine_op_label(eng._h, i).decode()


def _targs(kernel):
    return kernel.split("<", 1)[1].rstrip(">").split(", ")


def _assert_family(leg, C, B, kern, layers, maps):
    """The ops of the leg's family really run it (a leg cannot pass vacuously)."""
    knobs = LEGS[leg]
    for label in layers:
        assert kern.get(label), (label, kern)
    s1 = [k for k, l in layers.items() if l.kind == "conv" and l.segs[0][1].shape[2] == 3 and l.segs[0][2] == 1
          and k != HEADS_HIDDEN_LABEL]
    s2 = [k for k, l in layers.items() if l.kind == "conv" and l.segs[0][1].shape[2] == 3 and l.segs[0][2] == 2]
    up = [k for k, l in layers.items() if l.kind == "convt"]
    c3 = [k for k in kern.values() if k.startswith("tv::c3::conv3x3<")]
    if leg == "generic":
        bad = {k: v for k, v in kern.items() if v.startswith(HAND_WRITTEN)}
        assert not bad, bad
        assert all(v.startswith(("tv::pipe::conv_pipe<", "tv::conv_igemm<")) for k, v in kern.items() if k in layers)
    elif leg == "lat":
        rest = [k for k in s1 + s2 + [k for k in layers if k.endswith("root.conv")] if kern[k] and k != BLOCK0_CONV1]
        not_lat = {k: kern[k] for k in rest if not kern[k].startswith("tv::lat::conv_lat<")}
        assert not not_lat, not_lat
    elif leg == "burst":
        n = sum(v.startswith("tv::burst::conv_burst<") for v in kern.values())
        assert n >= 10, kern
    elif leg != "default":  # the halo legs
        for k in s1:
            assert kern[k].startswith("tv::c3::conv3x3<"), (k, kern[k])
            assert _targs(kern[k])[7] == str(C // 32), kern[k]  # channel blocks of the body: 4, or 2 at C = 64
        hid = kern[HEADS_HIDDEN_LABEL]
        assert hid.startswith("tv::c3::conv3x3<"), hid
        fused = knobs.get("TV_HEADFUSE") != "0"
        assert _targs(hid)[4] == ("1" if fused else "0"), hid
        assert (kern[HEADS_OUT_LABEL] == "(fused into the 3x3 heads)") == fused, kern[HEADS_OUT_LABEL]
        if C == 128:
            ss2 = knobs.get("TV_STEMFUSE") != "0"
            for k in s2:
                want = "tv::ss2::stem_s2<" if ss2 and k == BLOCK0_CONV1 else "tv::c3s2::conv3x3s2<"
                assert kern[k].startswith(want), (k, kern[k])
            assert kern[STEM].startswith("(fused into" if ss2 else "tv::stem::stem_conv<"), kern[STEM]
            for k in up:
                assert kern[k].startswith("tv::convt::convt_add<"), (k, kern[k])
            if B == B_4PHASE:  # the s = 2 steps from 13x18 in groups of 4 phases, the smaller ones one by one
                assert _targs(kern[UP_S2])[1] == "4", kern[UP_S2]
                assert any(_targs(kern[k])[1] == "1" for k in up), [kern[k] for k in up]
        else:
            assert kern[STEM].startswith("tv::stem::stem_conv<"), kern[STEM]
            # the phantom unit: a two-channel-block layer whose unit count is odd (one 64-channel half
            # tile per pixel tile, TW x 512 / TW pixels)
            odd = []
            for k in s1:
                a = _targs(kern[k])
                tw, nw = int(a[2]), int(a[-1])
                th = 64 * nw // tw
                h, w = maps[k]
                odd.append((B * -(-h // th) * -(-w // tw)) % 2 == 1)
            assert any(odd), "no layer with an odd unit count: choose another B"
        if "TV_C3_TW" in knobs:
            assert all(_targs(k)[2] == knobs["TV_C3_TW"] for k in c3), c3
        if "TV_C3_NI" in knobs:
            assert all(_targs(kern[k])[6] == knobs["TV_C3_NI"] for k in s1), [kern[k] for k in s1]
        if "TV_C3_NW" in knobs:
            assert all(_targs(k)[-1] == "8" for k in c3), c3


def _run(monkeypatch, leg, C, geometry, precision, B=None, u8=False):
    from tauv_vision_amd import engine as E
    t0 = time.time()
    h, w, b0 = GEOMETRIES[geometry]
    B = B or b0
    monkeypatch.setattr(E, "_DIAG_KNOBS", dict(LEGS[leg]))
    sd = _weights(C)
    model = LR.make_model(C, precision)[0].cuda()
    frames, img = LR.case_frames(h, w, B)
    x = frames.cuda() if u8 else img.cuda()
    eng = model.engine(torch.device("cuda", 0), h, w)
    ops = eng.op_outputs(x)
    torch.cuda.synchronize()
    kern = {label: k for label, k, _ in ops}
    stored = {label: (None if t is None else LR.nchw64(t)) for label, _, t in ops}
    layers = LR.layer_graph(sd, LR.HEIGHTS, LR.DOWNSAMPLES)
    maps = {label: tuple(t.shape[2:]) for label, t in stored.items() if t is not None}
    _assert_family(leg, C, B, kern, layers, maps)
    rep = LR.check(sd, LR.HEIGHTS, LR.DOWNSAMPLES, img.double(), precision, stored, kern)
    det, stat = rep.worst()
    key = f"layers/{leg}/C{C}/{geometry}/B{B}/{precision}" + ("/u8" if u8 else "")
    # the normal forward (grouped launches, the graph path as it is) against the un-hooked oracle
    pred = model.forward_frames(x) if u8 else model(x)
    ref = _oracle(C, h, w, B)
    end2end = {}
    for f, r in ref.items():
        got = getattr(pred, f).detach().cpu().double()
        end2end[f] = float((got - r).abs().max()) / max(1.0, float(r.abs().max()))
    took = time.time() - t0
    record_measurement(key, {"det_ratio": det, "stat_ratio": stat, "c": LR.C_STAT[precision], "end_to_end": end2end,
                             "not_stored": rep.skipped, "seconds": took})
    print(f"{key}: {det:.3f} x deterministic, {stat:.3f} x u(|ref|+Q) (c = {LR.C_STAT[precision]:.2f}), "
          f"{len(rep.rows)} layers compared, {len(rep.skipped)} not stored, end to end "
          f"{max(end2end.values()):.2e}, {took:.1f} s")
    fails = rep.failures(LR.C_STAT[precision])
    assert not fails, "\n".join(fails)
    for f, e in end2end.items():
        assert e <= fwd.TOL[precision], (f, e)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("geometry", ["G1", "G2", "G3"])
@pytest.mark.parametrize("leg", ["default", "halo"])
def test_layers_default_and_halo(monkeypatch, leg, geometry, precision):
    _run(monkeypatch, leg, 128, geometry, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_layers_halo_u8_frames(monkeypatch, precision):
    """The u8 frames mode of the stem (the fp32 NCHW mode is every other case)."""
    _run(monkeypatch, "halo", 128, "G1", precision, u8=True)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_layers_persistent_workgroups_walk_units(monkeypatch, precision):
    """8 CUs: every persistent workgroup walks several units, across frames, with uneven shares."""
    _run(monkeypatch, "cus8", 128, "G1", precision)


def test_layers_convt_four_phase_groups(monkeypatch):
    from tauv_vision_amd import engine as E
    monkeypatch.setattr(E, "_DIAG_KNOBS", dict(CUS8))
    h, w, _ = GEOMETRIES["G1"]
    eng = LR.make_model(128, "fp16")[0].cuda().engine(torch.device("cuda", 0), h, w)
    n = len(eng.op_shapes(B_4PHASE - 1))  # (plans the 17-frame workspace)
    # one frame fewer: only the s = 4 step (16 phases) reaches groups of 4, no s = 2 step does
    four = [_lib_label(eng, i) for i, k in enumerate(eng.op_kernels(B_4PHASE - 1, n))
            if k.startswith("tv::convt::convt_add<") and _targs(k)[1] == "4"]
    assert four == [UP_S4], four
    del eng
    _run(monkeypatch, "cus8", 128, "G1", "fp16", B=B_4PHASE)


@pytest.mark.parametrize("leg", [k for k in LEGS if k.startswith("cus8+")])
def test_layers_kernel_variants(monkeypatch, leg):
    _run(monkeypatch, leg, 128, "G1", "fp16")


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_layers_64_channel_body_phantom_unit(monkeypatch, precision):
    _run(monkeypatch, "cus8", 64, "G1", precision)


@pytest.mark.parametrize("geometry", ["G1", "G3"])
@pytest.mark.parametrize("leg", ["lat", "burst", "generic"])
def test_layers_other_routes(monkeypatch, leg, geometry):
    _run(monkeypatch, leg, 128, geometry, "fp16")


def test_tap_reports_what_is_stored_and_changes_nothing():
    """tv_engine_op_outputs: ops done inside another launch store nothing, the last op's tensor is
    the forward's output bit for bit (one op per launch == the grouped schedule), bad arguments are
    TV_EINVAL with a message."""
    import ctypes
    from tauv_vision_amd import _lib
    h, w, B = GEOMETRIES["G3"]
    model = LR.make_model(128, "fp16")[0].cuda()
    x = LR.case_frames(h, w, B)[1].cuda()
    eng = model.engine(torch.device("cuda", 0), h, w)
    before = eng.forward(x).clone()
    ops = eng.op_outputs(x)
    by_label = {label: (k, t) for label, k, t in ops}
    assert by_label[STEM][1] is None and by_label[STEM][0].startswith("(fused into")
    assert by_label[HEADS_HIDDEN_LABEL][1] is None
    assert by_label[BLOCK0_CONV1][1].shape == (B, (h + 1) // 2, (w + 1) // 2, 128)
    assert by_label[BLOCK0_CONV1][1].dtype == torch.float16
    assert ops[-1][2].dtype == torch.float32 and torch.equal(ops[-1][2], before)
    assert torch.equal(eng.forward(x), before)
    L = _lib.lib()
    assert L.tv_engine_op_outputs(None, None, 0, B, None, None, None, 0) == _lib.TV_EINVAL
    assert L.tv_engine_op_outputs(eng._h, ctypes.c_void_p(x.data_ptr()), 0, B, None, None, None, 0) == _lib.TV_EINVAL
    assert L.tv_last_error()
    n = ctypes.c_int32()
    assert L.tv_engine_op_shapes(eng._h, 0, None, None, 0, ctypes.byref(n)) == _lib.TV_EINVAL
