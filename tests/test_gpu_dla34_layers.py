"""Every op of the native CenterpointDLA34 plan (TV_ARCH_DLA34) on its own, at odd sizes, against float64,
on its routes.

tests/dla34_layer_ref.py has the graph, the bounds and their derivation per op kind;
tests/test_dla34_layer_ref_cpu.py shows on the CPU that the graph is oracle.ref_dla34 to 1e-9, that the
injected faults (root segments misordered or at the wrong ci0, floor-mode and over-reading pooling, the
residual from the un-pooled input, a dropped level_root child, the pad_to_match shift on the wrong axis
or dropped, transposed or mis-padded depthwise taps, four DCN sampling faults) break both bounds, and
measures the statistical constant: c_measured = 1.84 (fp16) / 1.85 (bf16), asserted here at twice that
(dla34_layer_ref.C_STAT_DLA34 = 3.68 / 3.70). fp32 is judged by the deterministic bound alone.

Model: tv.CenterpointDLA34, plain 4-label heads [4, 2, 2], seeded weights over the reference key list.
Geometries (dla34_layer_ref.GEOMETRIES; the planner needs >= 32 each way; maps per side: 100: 50, 25, 13,
7, 4; 140: 70, 35, 18, 9, 5; 148: 74, 37, 19, 10, 5; 76: 38, 19, 10, 5, 3; 104: 52, 26, 13, 7, 4; 36: 18, 9,
5, 3, 2; 44: 22, 11, 6, 3, 2):
  G1  100x140 B=3  sy = 1, sx = 0 on the f = 4 step; partial tiles both ways
  G1T 140x100 B=2  sy = 0, sx = 1
  G2  148x76  B=1  width under one 32-wide tile
  G3  36x44   B=5  every map inside one tile; B h w no multiple of 32
  G4  100x104 B=1  sy = sx = 1
Each case asserts the planned map sizes and the f = 4 step's (sy, sx) from the stored tensors before it
compares anything, then from the kernel names that the leg's family runs (_assert_family: every DCN row's
kernel instance and split-K slice count is the one pass_dcn / launch_dcn_gemm must choose for the layer's
B H W, C, N, the CU count and the knobs). Each case also runs the normal grouped forward against the
un-hooked float64 oracle under test_gpu_dla34.TOL, so an arena lifetime that the one-op-per-launch tap
hides still shows.

Legs (engine._DIAG_KNOBS): LEGS below. conv_small has no knob that turns it off: the generic leg keeps it
on the three narrow layers and asserts every other conv on the generic GEMMs, DCN fused through dcn_gemm.

Measured on MI355X (largest ratio over the layers of each leg: x deterministic bound / x statistical scale,
then the same over the matrix ops alone -- conv and DCN rows: the rounding-only ops (staging, the
up-sampling add) reach ~1.0 x their bound by construction -- then the largest end-to-end error of the
grouped forward; recorded per case under "layers/dla34/..." by helpers.record_measurement):
  default              fp16  0.998 / 1.958   0.514 / 1.958   1.2e-04  G1 B3, G1T B2, G2 B1, G3 B5, G4 B1
  default              bf16  0.996 / 1.876   0.563 / 1.876   7.5e-04  G1 B3, G1T B2, G2 B1, G3 B5, G4 B1
  default              fp32  0.996 / (36)    0.021 / (36.2)  1.2e-07  G2 B1, G4 B1   (statistical ratio not asserted)
  halo                 fp16  0.998 / 1.958   0.514 / 1.958   1.2e-04  G1 B3, G1 B3 u8, G1T B2, G2 B1, G3 B5, G4 B1
  halo                 bf16  0.996 / 1.876   0.563 / 1.876   7.8e-04  G1 B3, G1T B2, G2 B1, G3 B5, G4 B1
  cus8                 fp16  0.997 / 1.958   0.514 / 1.958   1.0e-04  G1 B3, G3 B5, G4 B1
  cus8                 bf16  0.996 / 1.876   0.563 / 1.876   7.9e-04  G1 B3, G3 B5, G4 B1
  TV_DCN_SPLIT=0       fp16  0.999 / 1.958   0.514 / 1.958   1.0e-04  G1 B3, G4 B1
  TV_DCN_SPLIT=9       fp16  0.997 / 1.958   0.514 / 1.958   9.9e-05  G1 B3, G4 B1
  TV_DCN64=0           fp16  0.999 / 1.805   0.514 / 1.805   1.0e-04  G1 B3
  TV_DCN64=0           bf16  0.996 / 1.876   0.524 / 1.876   7.7e-04  G1 B3
  TV_DCN64=2           fp16  0.997 / 1.805   0.514 / 1.805   1.1e-04  G1 B3
  TV_DCN64=2           bf16  0.996 / 1.876   0.524 / 1.876   7.5e-04  G1 B3
  TV_DCN64=3           fp16  0.999 / 1.805   0.514 / 1.805   1.0e-04  G1 B3
  TV_DCN64=3           bf16  0.996 / 1.876   0.524 / 1.876   7.7e-04  G1 B3
  TV_DCN64=5           fp16  0.999 / 1.805   0.514 / 1.805   1.0e-04  G1 B3
  TV_DCN64=5           bf16  0.996 / 1.876   0.524 / 1.876   7.7e-04  G1 B3
  lat                  fp16  0.998 / 1.806   0.514 / 1.806   1.0e-04  G1 B3, G3 B5
  burst                fp16  0.999 / 1.805   0.514 / 1.805   1.2e-04  G1 B3, G3 B5
  halo+TV_C1X1=0       fp16  0.998 / 1.814   0.514 / 1.814   1.1e-04  G1 B3, G3 B5
  generic              fp16  0.997 / 1.813   0.514 / 1.813   1.5e-04  G1 B3, G3 B5
  TV_PIPE_SPLIT=0      fp32  0.997 / (28)    0.031 / (27.8)  1.1e-07  G4 B1
  two slices           fp16  0.992 / 1.698   0.482 / 1.698   1.2e-04  G3 B16 (8 + 8: slice_min = 8)
Per op kind over all 16-bit cases: conv rows 0.514 / 1.958 (fp16) and 0.563 / 1.876 (bf16); the fused DCN rows
0.337 / 0.702 and 0.349 / 1.192 (their bound carries r = 2 and the 1e-4 sigmoid bar); dwconvt_add 0.999 /
0.999 and 0.996 / 0.996 (0.997 in fp32: one rounding of the fp64 sum, ~1.0 by construction); the fp32
dcn_sample rows 0.197 of their bound; the stored staging (generic leg) 0.939; maxpool2_ceil exact.
One fault was found and fixed. dwconvt_add summed its taps and the skip value in fp32: where they nearly cancel
the result lost its relative accuracy. halo / G1T / bf16, `model.ida_up.up_1+pad_to_match+add`, (b=1, y=14, x=6,
channel 20): ref = -2.896e-9 where A = 2.447e-2, got = -2.969e-9, 6.43 x u |ref| against c = 3.80 (inside the
then deterministic bound, which carried 5 2^-24 A). The kernel now sums in fp64 (dla34.hip) and every up-sampling
add is within one rounding of float64 (<= 0.999 x u |ref|). Cost: DLA-34 at B = 64, 6436-6458 -> 6234-6239
frames/s (two interleaved runs each, same box); R18 has no such op.
Nothing else was found: every layer of every leg is inside both bounds, every family assertion holds, every
planned (sy, sx) is the geometry's.
Slowest case: default/G1/B3/fp16 1.2-1.6 s (the first case: it also computes the shared float64 oracle); every
other case at most 1.1 s.
The recorded files: profiles/layers/dla34_layers_gpu.json (this table's cases and tests/test_gpu_dla34_aux.py's),
profiles/layers/layers_cpu.json (c).
"""
import functools
import time

import pytest
import torch

import dla34_layer_ref as DL
import layer_ref as LR
import test_gpu_dla34 as TD
import test_gpu_layers as TL
from helpers import record_measurement

pytestmark = pytest.mark.gpu

HALO, CUS8 = TL.HALO, TL.CUS8
LEGS = {
    "default": {},
    "halo": HALO,
    "cus8": CUS8,
    "TV_DCN_SPLIT=0": {"TV_DCN_SPLIT": "0"},
    "TV_DCN_SPLIT=9": {"TV_DCN_SPLIT": "9"},
    "TV_DCN64=0": {"TV_DCN64": "0"},
    "TV_DCN64=2": {"TV_DCN64": "2"},
    "TV_DCN64=3": {"TV_DCN64": "3"},
    "TV_DCN64=5": {"TV_DCN64": "5"},
    "lat": TL.LEGS["lat"],
    "burst": TL.LEGS["burst"],
    "halo+TV_C1X1=0": dict(HALO, TV_C1X1="0"),
    "generic": dict(TL.LEGS["generic"], TV_DCN64="0"),
    "TV_PIPE_SPLIT=0": {"TV_PIPE_SPLIT": "0"},
}
GEMM_T = {"fp16": "_Float16", "bf16": "__bf16", "fp32": "float"}
PIPE, IGEMM, LAT, BURST, C3 = ("tv::pipe::conv_pipe<", "tv::conv_igemm<", "tv::lat::conv_lat<", "tv::burst::conv_burst<",
                               "tv::c3::conv3x3<")
FUSED_SAMPLING = "(sampled inside the fused DCNv2 kernel)"
FIELDS = {"heatmap": slice(0, 4), "size": slice(4, 6), "offset": slice(6, 8)}


@functools.lru_cache(maxsize=None)
def _graph():
    sd = DL.seeded_weights()[1]
    return sd, DL.dla34_layers(sd)


@functools.lru_cache(maxsize=None)
def _oracle(geometry, B):
    """The un-hooked float64 oracle of a case: computed once, shared by every leg."""
    h, w, _ = DL.GEOMETRIES[geometry]
    return DL.oracle_heads(_graph()[0], LR.case_frames(h, w, B)[1].double())


def _expected_dcn(knobs, precision, M, C, N, cu):
    """The kernel instance pass_dcn + launch_dcn_gemm choose for a fused DCN layer of M = B H W pixels."""
    t = GEMM_T[precision]
    mode = int(knobs.get("TV_DCN64", 1))
    wide = N % 128 == 0
    if mode in (3, 4) and C == 64 and N == 64:
        return f"tv::dcn::dcn_win<{t}>"
    if mode == 5 and C % 64 == 0:
        return f"tv::dcn::dcn_gemm64d<{t}, {128 if wide else 64}, 64>"
    if mode and C % 64 == 0:
        bn = 128 if wide else 64
        px = 64 if (not wide or mode == 2 or -(-M // 128) * (N // 128) < 1024) else 128
        name = f"tv::dcn::dcn_gemm64<{t}, {bn}, {px}>"
        split_max = max(0, min(9, int(knobs.get("TV_DCN_SPLIT", 4))))
        if split_max >= 2 and mode in (1, 2):
            units = -(-M // px) * (N // bn)
            ks = min(split_max, cu // max(1, units))
            if ks >= 2:
                name += f" split-K {ks}"
        return name
    return f"tv::dcn::dcn_gemm<{t}, {128 if wide else 64}>"


def _assert_family(leg, precision, B, kern, layers, stored):
    """The ops of the leg's family really run it (a leg cannot pass vacuously)."""
    knobs = LEGS[leg]
    for label in layers:
        assert kern.get(label), (label, kern)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    if "TV_CUS" in knobs:
        cu = max(8, min(cu, int(knobs["TV_CUS"])))
    t = GEMM_T[precision]
    convs = [k for k, l in layers.items() if l.kind == "conv"]
    roots = [k for k in convs if k.endswith(".root.conv")]
    deep = [k for k in convs if k.startswith(("model.base.level3", "model.base.level4", "model.base.level5"))]
    n_split = 0
    for k, l in layers.items():
        if l.kind == "maxpool":
            assert kern[k] == f"tv::dla::maxpool2_ceil<{t}>", (k, kern[k])
        elif l.kind == "dwconvt":
            assert kern[k] == f"tv::dla::dwconvt_add<{t}>", (k, kern[k])
        elif l.kind == "dcn_sample":
            if precision == "fp32":
                assert kern[k] == "tv::dla::dcn_sample<float>" and stored[k] is not None, (k, kern[k])
            else:
                assert kern[k] == FUSED_SAMPLING and stored[k] is None, (k, kern[k])
        elif l.kind == "dcn":
            if precision == "fp32":
                assert kern[k].startswith((PIPE, IGEMM, LAT)), (k, kern[k])
                continue
            x = stored[l.srcs[0]]
            want = _expected_dcn(knobs, precision, x.shape[0] * x.shape[2] * x.shape[3], x.shape[1], l.w.shape[0], cu)
            assert kern[k] == want, (k, kern[k], want)
            n_split += " split-K " in kern[k]
    if precision == "fp32":
        pipe = [kern[k] for k in convs if kern[k].startswith(PIPE)]
        assert not any(v.startswith(("tv::dcn::", "tv::c3", "tv::csm::", "tv::stem::", BURST)) for v in kern.values())
        if knobs.get("TV_PIPE_SPLIT") == "0":
            assert pipe and not any(" split-K " in v for v in pipe), pipe
        else:
            assert any(" split-K " in v for v in pipe), pipe
        return
    mode = int(knobs.get("TV_DCN64", 1))
    # (every row's slice count is already the expected one; here: the leg is not vacuous)
    if knobs.get("TV_DCN_SPLIT") == "0" or mode not in (1, 2):
        assert n_split == 0, n_split
    elif "TV_CUS" not in knobs:  # (8 CUs: only a layer of at most 4 work units still splits)
        assert n_split > 0, "no DCN layer runs split-K: choose another geometry"
        if knobs.get("TV_DCN_SPLIT") == "9":
            assert any(int(v.rsplit(" ", 1)[1]) > 4 for v in kern.values() if " split-K " in v and "::dcn::" in v), kern
    if mode == 3:
        win = [k for k, v in kern.items() if v.startswith("tv::dcn::dcn_win<")]
        c64 = [k for k, l in layers.items() if l.kind == "dcn" and l.w.shape[0] == 64 and l.w.shape[1] == 64]
        assert win == c64 and win, (win, c64)
    if leg in ("halo", "cus8", "halo+TV_C1X1=0"):
        assert not any(v.startswith((LAT, BURST)) for v in kern.values()), kern
        assert sum(v.startswith(C3) for v in kern.values()) >= 30, kern  # (the trees' and the offset + mask 3x3 convs)
        c1 = [k for k in roots if kern[k].startswith("tv::c1x1::conv1x1_stream<")]
        if knobs.get("TV_C1X1") == "0":
            assert not any(v.startswith("tv::c1x1::") for v in kern.values())
            assert all(kern[k].startswith((PIPE, IGEMM)) for k in roots), [kern[k] for k in roots]
        else:
            assert c1, [kern[k] for k in roots]
    elif leg == "lat":
        not_lat = {k: kern[k] for k in deep if not kern[k].startswith(LAT)}
        assert not not_lat, not_lat
    elif leg == "burst":
        n = sum(v.startswith(BURST) for v in kern.values())
        assert n >= 10, kern
    elif leg == "generic":
        hand = tuple(p for p in TL.HAND_WRITTEN) + ("tv::ct3::",)
        bad = {k: v for k, v in kern.items() if v.startswith(hand)}
        assert not bad, bad
        rest = [k for k in convs if not kern[k].startswith("tv::csm::")]
        assert all(kern[k].startswith((PIPE, IGEMM)) for k in rest), {k: kern[k] for k in rest}
        assert len(convs) - len(rest) <= 3  # conv_small's three narrow layers: no knob turns it off


def _assert_geometry(geometry, stored, layers):
    """The planned maps and the f = 4 step's shift are the ones the geometry was chosen for."""
    h, w, _ = DL.GEOMETRIES[geometry]
    sizes = {tuple(v.shape[2:]) for v in stored.values() if v is not None}
    for mh, mw in zip(DL.MAPS[h], DL.MAPS[w]):
        assert (mh, mw) in sizes, (geometry, mh, mw)
    geo = DL.up_geometry(layers[DL.UP_F4], stored)
    assert geo[:4] == (DL.MAPS[h][3], DL.MAPS[w][3], DL.MAPS[h][1], DL.MAPS[w][1]), geo
    if geometry in DL.SHIFT_F4:
        assert geo[4:] == DL.SHIFT_F4[geometry], (geometry, geo)


def _tap(eng, x):
    ops = eng.op_outputs(x)
    torch.cuda.synchronize()
    labels = DL.unique_labels([label for label, _, _ in ops])
    kern = {lb: k for lb, (_, k, _) in zip(labels, ops)}
    stored = {lb: (None if t is None else LR.nchw64(t)) for lb, (_, _, t) in zip(labels, ops)}
    return kern, stored, ops[-1][2]


def _end_to_end(out, ref, precision):
    got = LR.nchw64(out)
    e = {f: float((got[:, s] - ref[:, s]).abs().max()) / max(1.0, float(ref[:, s].abs().max())) for f, s in FIELDS.items()}
    return e


def _run(monkeypatch, leg, geometry, precision, B=None, u8=False):
    from tauv_vision_amd import engine as E
    t0 = time.time()
    h, w, b0 = DL.GEOMETRIES[geometry]
    B = B or b0
    monkeypatch.setattr(E, "_DIAG_KNOBS", dict(LEGS[leg]))
    sd, layers = _graph()
    model = DL.make_model(precision).cuda()
    frames, img = LR.case_frames(h, w, B)
    x = frames.cuda() if u8 else img.cuda()
    eng = model.engine(torch.device("cuda", 0), h, w)
    kern, stored, _ = _tap(eng, x)
    assert sorted(kern) == sorted(layers), (sorted(set(kern) ^ set(layers)))
    _assert_geometry(geometry, stored, layers)
    _assert_family(leg, precision, B, kern, layers, stored)
    with torch.no_grad():
        rep = DL.check(layers, img.double(), precision, stored, kern)
    assert rep.up[DL.UP_F4] == DL.up_geometry(layers[DL.UP_F4], stored)
    # the normal forward (grouped launches, the schedule as it is) against the un-hooked oracle
    out = eng.forward_u8(x) if u8 else eng.forward(x)
    torch.cuda.synchronize()
    end2end = _end_to_end(out, _oracle(geometry, B), precision)
    _finish(f"layers/dla34/{leg}/{geometry}/B{B}/{precision}" + ("/u8" if u8 else ""), t0, rep, precision, kern, layers,
            end2end)


def _finish(key, t0, rep, precision, kern, layers, end2end):
    det, stat = rep.worst()
    mm = [r for r in rep.rows if layers[r[0]].kind in ("conv", "dcn")]
    mm_det, mm_stat = max(r[3] for r in mm), max(r[4] for r in mm)
    by_kind = {}
    for r in rep.rows:  # (largest ratios per op kind: the DCN GEMMs and the up-sampling adds on their own too)
        k = layers[r[0]].kind
        by_kind[k] = [max(a, b) for a, b in zip(by_kind.get(k, [0.0, 0.0]), r[3:5])]
    took = time.time() - t0
    fams = {}
    for v in kern.values():
        f = v.split("<", 1)[0]
        fams[f] = fams.get(f, 0) + 1
    c = DL.C_STAT_DLA34.get(precision)
    not_stored = [k for k in rep.skipped if layers[k].kind != "dcn_sample"]
    record_measurement(key, {"det_ratio": det, "stat_ratio": stat, "conv_det_ratio": mm_det, "conv_stat_ratio": mm_stat,
                             "c": c, "by_kind": by_kind, "end_to_end": end2end, "not_stored": not_stored,
                             "dcn_sampling_not_stored": len(rep.skipped) - len(not_stored), "kernels": fams,
                             "seconds": took})
    print(f"{key}: {det:.3f} x deterministic, {stat:.3f} x statistical scale (c = {c}; matrix ops {mm_det:.3f} / "
          f"{mm_stat:.3f}), {len(rep.rows)} layers compared, {len(rep.skipped)} not stored, end to end "
          f"{max(end2end.values()):.2e}, {took:.1f} s")
    fails = rep.failures(c if c is not None else float("inf"))
    assert not fails, "\n".join(fails)
    for f, e in end2end.items():
        assert e <= TD.TOL[precision], (f, e)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("geometry", list(DL.GEOMETRIES))
@pytest.mark.parametrize("leg", ["default", "halo"])
def test_layers_default_and_halo(monkeypatch, leg, geometry, precision):
    _run(monkeypatch, leg, geometry, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("geometry", ["G1", "G3", "G4"])
def test_layers_persistent_workgroups_walk_units(monkeypatch, geometry, precision):
    """8 CUs: the persistent conv kernels walk several units; DCN split-K only where <= 4 units are left."""
    _run(monkeypatch, "cus8", geometry, precision)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("leg", ["TV_DCN64=0", "TV_DCN64=2", "TV_DCN64=3", "TV_DCN64=5"])
def test_layers_dcn_kernel_variants(monkeypatch, leg, precision):
    _run(monkeypatch, leg, "G1", precision)


@pytest.mark.parametrize("geometry", ["G1", "G4"])
@pytest.mark.parametrize("leg", ["TV_DCN_SPLIT=0", "TV_DCN_SPLIT=9"])
def test_layers_dcn_split_k(monkeypatch, leg, geometry):
    _run(monkeypatch, leg, geometry, "fp16")


@pytest.mark.parametrize("geometry", ["G1", "G3"])
@pytest.mark.parametrize("leg", ["lat", "burst", "halo+TV_C1X1=0", "generic"])
def test_layers_other_routes(monkeypatch, leg, geometry):
    _run(monkeypatch, leg, geometry, "fp16")


def test_layers_halo_u8_frames(monkeypatch):
    """The u8 frames mode of the stem (the fp32 NCHW mode is every other case)."""
    _run(monkeypatch, "halo", "G1", "fp16", u8=True)


@pytest.mark.parametrize("leg,geometry", [("default", "G2"), ("default", "G4"), ("TV_PIPE_SPLIT=0", "G4")])
def test_layers_fp32(monkeypatch, leg, geometry):
    """The fp32 plan: DcnSample stores the 9 C-channel columns, the GEMM runs over them; conv_pipe split-K on and off."""
    _run(monkeypatch, leg, geometry, "fp32")


def test_layers_across_the_slice_boundary(monkeypatch):
    """G3 at the smallest batch the engine runs as two concurrent slices: the per-layer tap at the slice
    size on each half (the workspace each slice runs in), and the two-slice forward equal to the two taps'
    outputs bit for bit, frame for frame, across the boundary."""
    from tauv_vision_amd import engine as E
    t0 = time.time()
    monkeypatch.setattr(E, "_DIAG_KNOBS", {})
    h, w, _ = DL.GEOMETRIES["G3"]
    sd, layers = _graph()
    model = DL.make_model("fp16").cuda()
    eng = model.engine(torch.device("cuda", 0), h, w)
    B = next(b for b in range(2, 65) if len(eng.slices(b)) > 1)
    sizes = eng.slices(B)
    slice_min = B // 2
    assert sizes == [slice_min, slice_min] and eng.slices(B - 1) == [B - 1], (B, sizes)
    _, img = LR.case_frames(h, w, B)
    x = img.cuda()
    out = eng.forward(x)
    torch.cuda.synchronize()
    f0 = 0
    for n in sizes:
        part = x[f0:f0 + n].contiguous()
        kern, stored, last = _tap(eng, part)
        assert torch.equal(last, out[f0:f0 + n]), f"frames {f0}..{f0 + n - 1}: the slice's output differs from its tap"
        with torch.no_grad():
            rep = DL.check(layers, img[f0:f0 + n].double(), "fp16", stored, kern)
        _assert_family("default", "fp16", n, kern, layers, stored)
        fails = rep.failures(DL.C_STAT_DLA34["fp16"])
        assert not fails, "\n".join(fails)
        f0 += n
    end2end = _end_to_end(out, _oracle("G3", B), "fp16")
    _finish(f"layers/dla34/slices/G3/B{B}/fp16", t0, rep, "fp16", kern, layers, end2end)
