"""convt.hip (ConvTranspose2d(k = s, stride s) + pad_to_match + skip add) after its global accesses
were reshaped to whole pixel rows: the bytes it writes are the bytes the generic route writes.

The kernel now takes pixels as the MFMA rows, so that a wave's skip loads and stores cover the whole
256 B of a target pixel; only the routing of bytes changed, the arithmetic ((acc + bias) + skip in
fp32, one rounding, K in the same order) did not. Every case therefore asks for three things:

  * bit equality (torch.equal on the raw fp16 / bf16 tensors) with the same op on the TV_CONVT=0 route,
    which must be tv::pipe::conv_pipe (its mode-1 epilogue, the same arithmetic order);
  * the per-layer float64 bounds of tests/layer_ref.py (deterministic bound, and the statistical one
    at layer_ref.C_STAT) for the up-step on its own: the oracle's layer evaluated on the tensors the
    engine stored for the step's inputs (r = 1: only the weights are rounded);
  * the same forward twice gives identical bytes.

Each case asserts from the kernel names that the convt_add<T, NP> instance it is about ran.

Cases (128 channels, convt_supported's only size; the smallest shapes that reach each path). Engine
cases are tv.Centernet(tv.DLABackbone([1] * n, [128] * (n + 1), 2)) models, a level being ceil(previous / 2):
  exact cover     frame 24x40, n = 3: maps 6x10, 3x5, 2x3, 1x2. s = 2 from 3x5 onto 6x10 at B = 1, 2, 3:
                  M = 15 / 30 / 45 source pixels, never a whole 32-pixel tile; NP = 1. The same model runs
                  IDAUpReverse's s = 4 on the 2x3 map (B = 2 is the issue's large-stride case for s = 4).
  large strides   s = 8 on a 2x3 map: frame 64x96, n = 4; s = 16 on a 2x3 map: frame 128x192, n = 5; B = 2.
                  A wave's target pixels lie 2 and 4 KiB apart (1 KiB at s = 4).
  four phases     TV_CUS = 8, frame 320x424, n = 3, B = 2: s = 2 from 40x53 (4240 pixels = 132 tiles and a
                  half) onto 80x106; convt_schedule takes NP = 4 from 128 tiles on. Also through
                  tv_diag_convt_add with cus = 8.
  margin          a level is never smaller than half its target, so no plan has a target the up-sampled
                  map does not cover: these go through tv_diag_convt_add. s = 2, 3x5 onto 7x11 (the last
                  row and column uncovered) and onto 4x11 (pad_to_match's H-excess-pads-W quirk: shifted
                  one column right, cropped below, column 0 uncovered), B = 2, rows of 136 channels of
                  which 128 are written. Pixels outside the covered window keep the skip tensor's value
                  the caller put there, the 8 spare channels and the bytes behind the tensor stay
                  untouched. No generic route reaches these shapes either; their covered window is
                  compared bit for bit with the exact-cover launch on the same operands, which the
                  exact-cover case ties to the engine's op (tv_diag_convt_add on the op's stored inputs
                  and weights == the op's stored output) and through it to conv_pipe.
  grouped launch  the R18 golden geometry (480x640) at B = 2: the latency schedule runs up-steps of one
                  level in one convt_add_group launch; outputs equal TV_LATGROUP=0 (one launch per op)
                  and TV_CONVT=0 bit for bit.

Bit equality with conv_pipe also held for the kernel before the reshaping on every case above (the
cases were run against a build with the earlier convt.hip), so no case needs a recorded exception.

Measured on MI355X, largest ratio over the 67 up-steps of the cases (x deterministic bound / x u(|ref|+Q)):
fp16 0.660 / 1.842 (c = 3.92), bf16 0.627 / 1.957 (c = 4.62); the same figures on the earlier kernel, as
the bytes are the same. Slowest case: the grouped launch, 3.4 s (two R18 engines at 480x640); every other
case at most 1.4 s.
"""
import ctypes
import functools

import pytest
import torch

import layer_ref as LR
import test_gpu_forward as fwd
from helpers import case_input
from recipe import normalize, seeded_u8_frames

pytestmark = pytest.mark.gpu

CONVT = "tv::convt::convt_add<"
PIPE = "tv::pipe::conv_pipe<"
C = 128
R18 = "r18_c128_b1_480x640"


def _np_of(kernel):
    assert kernel.startswith(CONVT), kernel
    return int(kernel.split("<", 1)[1].rstrip(">").split(", ")[1])


def _build(n_levels, precision):
    import tauv_vision_amd as tv
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A(False, None), A(False, None), A(False, None), False, False,
                                             None) for i in range(LR.N_LABELS)])
    return tv.Centernet(tv.DLABackbone([1] * n_levels, [C] * (n_levels + 1), LR.DOWNSAMPLES), oc, precision=precision)


@functools.lru_cache(maxsize=None)
def _weights(n_levels):
    """Seeded weights of the n_levels model (as layer_ref.make_model): (state dict, its float64 copy)."""
    from recipe import seeded_state_dict
    sd = seeded_state_dict([(k, tuple(v.shape)) for k, v in _build(n_levels, "fp16").state_dict().items()])
    return sd, {k: v.double() for k, v in sd.items() if v.dtype.is_floating_point}


def _ops(monkeypatch, n_levels, h, w, B, precision, knobs, twice=False):
    """{label: (kernel, stored NHWC tensor or None)} of one forward, one op per launch (a fresh model:
    the engine reads the knobs when it is created)."""
    from tauv_vision_amd import engine as E
    monkeypatch.setattr(E, "_DIAG_KNOBS", dict(knobs))
    model = _build(n_levels, precision)
    model.load_state_dict(_weights(n_levels)[0])
    model = model.eval().cuda()
    x = LR.case_frames(h, w, B)[1].cuda()
    eng = model.engine(torch.device("cuda", 0), h, w)
    ops = eng.op_outputs(x)
    torch.cuda.synchronize()
    got = {label: (k, None if t is None else t.clone()) for label, k, t in ops}
    if twice:  # repeatability: the same forward again, identical bytes in every stored tensor
        again = eng.op_outputs(x)
        torch.cuda.synchronize()
        for label, k, t in again:
            assert k == got[label][0] and (t is None) == (got[label][1] is None), label
            assert t is None or torch.equal(_bits(t), _bits(got[label][1])), f"{label}: two forwards differ"
    return got


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t


def _f64_check(layer, stored, precision, what):
    """The up-step on its own against float64, from the tensors the engine stored for its inputs."""
    xs = {s: LR.nchw64(stored[s]) for s in layer.sources()}
    ref = LR.evaluate(layer, xs)
    det, stat = LR.bounds(layer, xs, ref, precision, 1)
    rd, rs = LR.ratios(LR.nchw64(stored[layer.label]), ref, det, stat)
    rd, rs = float(rd.max()), float(rs.max())
    print(f"{what} {layer.label}: {rd:.3f} x deterministic, {rs:.3f} x u(|ref|+Q) (c = {LR.C_STAT[precision]:.2f})")
    assert rd <= 1.0 and rs <= LR.C_STAT[precision], (what, layer.label, rd, rs)


def _engine_case(monkeypatch, n_levels, h, w, B, precision, knobs, want):
    """Runs the model on convt.hip and on the TV_CONVT=0 route; `want` = [(s, (src h, w), (target H, W), NP)]
    up-steps that must be among the ops, on that instance. Returns (new ops, layers, sd)."""
    sd = _weights(n_levels)[1]
    layers = LR.layer_graph(sd, [1] * n_levels, LR.DOWNSAMPLES)
    new = _ops(monkeypatch, n_levels, h, w, B, precision, knobs, twice=True)
    ref = _ops(monkeypatch, n_levels, h, w, B, precision, dict(knobs, TV_CONVT="0"))
    ups = [k for k, l in layers.items() if l.kind == "convt"]
    assert ups and all(new[k][1] is not None for k in ups)
    seen = []
    for k in ups:
        layer = layers[k]
        src, skip = new[layer.segs[0][0]][1], new[layer.skip][1]
        assert new[k][0].startswith(CONVT), (k, new[k][0])
        assert ref[k][0].startswith(PIPE), (k, ref[k][0])
        seen.append((layer.segs[0][2], tuple(src.shape[1:3]), tuple(skip.shape[1:3]), _np_of(new[k][0])))
        # the step's inputs are the same bytes on both routes (every op before it matched), so are its outputs
        for s in layer.sources():
            assert torch.equal(_bits(new[s][1]), _bits(ref[s][1])), f"{k}: input {s} differs between the routes"
        assert torch.equal(_bits(new[k][1]), _bits(ref[k][1])), f"{k} [{new[k][0]}] differs from [{ref[k][0]}]"
        _f64_check(layer, {s: new[s][1] for s in layer.sources() + [k]}, precision, f"B={B} {precision}")
    print(f"{h}x{w} B={B} {precision}: up-steps (s, source, target, NP) {seen}")
    for step in want:
        assert step in seen, (step, seen)
    return new, layers, sd


def _diag(src, weight, bias, s, skip, out, tH, tW, sy, sx, precision, cus=0):
    """tv_diag_convt_add on device tensors (src [B, h, w, ldc], skip / out [B, tH, tW, ldc]); returns NP."""
    from tauv_vision_amd import _lib
    B, h, w, _ = src.shape
    wc, bc = weight.float().contiguous().cpu(), bias.float().contiguous().cpu()
    np_ = ctypes.c_int32(0)
    _lib.check(_lib.lib().tv_diag_convt_add(
        ctypes.c_void_p(src.data_ptr()), B, h, w, src.shape[3], ctypes.c_void_p(wc.data_ptr()),
        ctypes.c_void_p(bc.data_ptr()), s, ctypes.c_void_p(skip.data_ptr()), skip.shape[3],
        ctypes.c_void_p(out.data_ptr()), out.shape[3], tH, tW, sy, sx, _lib.DTYPES[precision], cus,
        ctypes.c_void_p(ctypes.addressof(np_)), _lib.stream_of(src.device)), "diag_convt_add")
    torch.cuda.synchronize()
    return np_.value


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("B", [1, 2, 3])
def test_exact_cover_partial_tile(monkeypatch, B, precision):
    new, layers, sd = _engine_case(monkeypatch, 3, 24, 40, B, precision, {},
                                   [(2, (3, 5), (6, 10), 1), (4, (2, 3), (6, 10), 1)])
    # the stand-alone entry on the op's own operands writes the op's bytes (ties the margin cases to this one)
    for k, layer in layers.items():
        if layer.kind != "convt":
            continue
        s = layer.segs[0][2]
        src, skip, got = new[layer.segs[0][0]][1], new[layer.skip][1], new[k][1]
        th, tw = skip.shape[1:3]
        # pad_to_match as the planner folds it into the target shift (the 4-tuple's H / W swap included)
        sy, sx = max(0, (src.shape[2] * s - tw) // 2), max(0, (src.shape[1] * s - th) // 2)
        out = skip.clone()
        n = _diag(src, layer.segs[0][1], layer.bias, s, skip, out, th, tw, sy, sx, precision)
        assert n == _np_of(new[k][0])
        assert torch.equal(_bits(out), _bits(got)), f"{k}: tv_diag_convt_add differs from the engine's op"


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("s,n_levels,h,w", [(8, 4, 64, 96), (16, 5, 128, 192)])
def test_large_strides(monkeypatch, s, n_levels, h, w, precision):
    """(s = 4 on a 2x3 map at B = 2 runs in test_exact_cover_partial_tile.)"""
    tgt = (h // 4, w // 4)
    _engine_case(monkeypatch, n_levels, h, w, 2, precision, {}, [(s, (2, 3), tgt, 1)])


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_four_phase_instance(monkeypatch, precision):
    _engine_case(monkeypatch, 3, 320, 424, 2, precision, {"TV_CUS": "8"}, [(2, (40, 53), (80, 106), 4)])


def _operands(B, h, w, s, tH, tW, precision, ldc, seed):
    """Seeded operands of a stand-alone up-step: skip / out rows of ldc >= 128 channels, the spare ones NaN."""
    dt = LR.TORCH_DTYPE[precision]
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, h, w, C, generator=g).to(dt)
    weight = torch.randn(C, C, s, s, generator=g) / C ** 0.5
    bias = torch.randn(C, generator=g)
    skip = torch.full((B, tH, tW, ldc), float("nan"), dtype=dt)
    skip[..., :C] = torch.randn(B, tH, tW, C, generator=g).to(dt)
    return src.cuda(), weight, bias, skip.cuda()


def _standalone_layer(weight, bias, s):
    return LR.Layer("up", "convt", [("src", weight.double(), s, 0)], bias.double(), 0, skip="skip", K=C)


TAIL = 4096  # elements behind the output that must stay untouched


def _run_standalone(src, weight, bias, s, skip, tH, tW, sy, sx, precision, cus=0):
    """out = the skip tensor's copy with NaN behind it; returns (out [B, tH, tW, ldc], NP)."""
    n = skip.numel()
    flat = torch.full((n + TAIL,), float("nan"), dtype=skip.dtype, device="cuda")
    flat[:n] = skip.reshape(-1)
    out = flat[:n].view(skip.shape)
    np_ = _diag(src, weight, bias, s, skip, out, tH, tW, sy, sx, precision, cus)
    assert torch.isnan(flat[n:].float()).all(), "wrote behind the output tensor"
    assert torch.isnan(out[..., C:].float()).all(), "wrote past the 128 channels of a row"
    return out, np_


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("tH,tW", [(7, 11), (4, 11)])
def test_uncovered_margin_and_shift(tH, tW, precision):
    B, h, w, s = 2, 3, 5, 2
    src, weight, bias, skip = _operands(B, h, w, s, tH, tW, precision, C + 8, seed=100 * tH + tW)
    sy, sx = max(0, (w * s - tW) // 2), max(0, (h * s - tH) // 2)  # (the planner's fold of pad_to_match)
    assert (sy, sx) == ((0, 0) if tH == 7 else (0, 1))
    out, np_ = _run_standalone(src, weight, bias, s, skip, tH, tW, sy, sx, precision)
    again, _ = _run_standalone(src, weight, bias, s, skip, tH, tW, sy, sx, precision)
    assert np_ == 1
    assert torch.equal(_bits(out[..., :C]), _bits(again[..., :C])), "two launches differ"
    # outside the covered window: the skip tensor, as it was
    y1, x1 = min(tH, sy + h * s), min(tW, sx + w * s)
    covered = torch.zeros(tH, tW, dtype=torch.bool)
    covered[sy:y1, sx:x1] = True
    assert (~covered).any()
    assert torch.equal(_bits(out[:, ~covered][..., :C]), _bits(skip[:, ~covered][..., :C]))
    # the covered window: the exact-cover launch (6x10 target, no shift) on the same operands, bit for bit
    win = skip[:, sy:sy + h * s, sx:sx + w * s].contiguous()
    if win.shape[1:3] == (h * s, w * s):
        full, _ = _run_standalone(src, weight, bias, s, win, h * s, w * s, 0, 0, precision)
    else:  # cropped below: the rows the target does not have read as zeros and are dropped again
        pad = torch.full((B, h * s, w * s, C + 8), float("nan"), dtype=skip.dtype, device="cuda")
        pad[..., :C] = 0
        pad[:, :win.shape[1], :win.shape[2], :C] = win[..., :C]
        full, _ = _run_standalone(src, weight, bias, s, pad, h * s, w * s, 0, 0, precision)
    assert torch.equal(_bits(out[:, sy:y1, sx:x1, :C]), _bits(full[:, :y1 - sy, :x1 - sx, :C]))
    stored = {"src": src, "skip": skip[..., :C], "up": out[..., :C]}
    _f64_check(_standalone_layer(weight, bias, s), stored, precision, f"{h}x{w} onto {tH}x{tW}")


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_four_phase_instance_standalone(precision):
    """40x53 at B = 2 on 8 CUs: 132 whole tiles and a half one, NP = 4; the same operands at the device's
    CU count run NP = 1 and must give the same bytes."""
    B, h, w, s = 2, 40, 53, 2
    src, weight, bias, skip = _operands(B, h, w, s, h * s, w * s, precision, C, seed=4053)
    out4, np4 = _run_standalone(src, weight, bias, s, skip, h * s, w * s, 0, 0, precision, cus=8)
    out1, np1 = _run_standalone(src, weight, bias, s, skip, h * s, w * s, 0, 0, precision)
    assert (np4, np1) == (4, 1), (np4, np1)
    assert torch.equal(_bits(out4), _bits(out1))
    _f64_check(_standalone_layer(weight, bias, s), {"src": src, "skip": skip, "up": out4}, precision, "NP = 4")


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_grouped_launch(monkeypatch, precision):
    """Up-steps of one level in one convt_add_group launch (the latency schedule at B <= 8)."""
    from tauv_vision_amd import engine as E
    H, W = case_input(R18).shape[-2:]
    x = normalize(seeded_u8_frames(2, H, W, seed=2).permute(0, 3, 1, 2).float() / 255.0).cuda()
    outs = {}
    for name, knobs in (("grouped", {}), ("again", {}), ("one per launch", {"TV_LATGROUP": "0"}),
                        ("generic", {"TV_CONVT": "0"})):
        monkeypatch.setattr(E, "_DIAG_KNOBS", dict(knobs))
        model = fwd.build(R18, precision)[0]
        if name in ("grouped", "generic"):
            eng = model.engine(torch.device("cuda", 0), H, W)
            n = len(eng.op_shapes(2))
            kern = [k for k in eng.op_kernels(2, n) if k.startswith((CONVT, PIPE))]
            assert any(k.startswith(CONVT) for k in kern) == (name == "grouped"), kern
        pred = model(x)
        outs[name] = {f: getattr(pred, f).detach().cpu() for f in fwd.FIELDS if getattr(pred, f) is not None}
    for name in ("again", "one per launch", "generic"):
        assert outs[name].keys() == outs["grouped"].keys()
        for f, t in outs["grouped"].items():
            assert torch.equal(t, outs[name][f]), f"{precision} {f}: grouped launch differs from {name}"
