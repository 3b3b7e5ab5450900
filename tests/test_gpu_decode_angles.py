"""tv_decode_angles (csrc/decode.hip) and what is built on it: DeviceAngleDecoder, decode_oriented_records,
decode_oriented, detect(..., angles=True) — against angle_decode_ref.py's float64 restatement of the
reference's angle_decode, under that module's bar (check_angles: the NaN pattern owed, and a circular
distance to float64 of at most max(4 * e_ref, 2^-20), e_ref the fp32 restatement's own error on the case)
and its condition on the bin logits (asserted on the inputs of every case).

Shapes: B=2, C=3, 5x7, K=6 (not square: a y / x swap reads another cell; labels of periods 2 pi, pi / 2 and
one untrained; an image with fewer records than K and one with none; the pitch head absent) and B=4, C=1,
9x11, K=70 (280 threads: a second, ragged block of the 256-thread launch). Heads in two view forms: channel
slices of one padded NHWC tensor (the native models' Prediction) and NCHW tensors permuted to NHWC (the
reference's)."""
import ctypes
from math import pi

import numpy as np
import pytest
import torch

import angle_decode_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
AXES = ("roll", "pitch", "yaw")
# counts: of the hand-made records; planted: peaks above the threshold per image at the API level (at most
# the cells of a 2-strided grid); ranges: rows roll, pitch, yaw (label 2 trains nothing, label 1 no roll)
SMALL = dict(B=2, C=3, H=5, W=7, K=6, counts=(4, 0), planted=(4, 0), absent=("pitch",),
             ranges=[[pi, np.nan, np.nan], [pi, pi, np.nan], [2 * pi, pi / 2, np.nan]])
WIDE = dict(B=4, C=1, H=9, W=11, K=70, counts=(70, 33, 0, 69), planted=(30, 17, 0, 29), absent=(),
            ranges=[[2 * pi], [pi / 2], [pi]])
_CASES = {}


def _config(ranges):
    """The ObjectConfigSet whose angle_ranges() is `ranges` [3, C] (NaN: the label does not train the axis)."""
    import tauv_vision_amd as tv
    A = tv.AngleConfig
    cfgs = []
    for c in range(len(ranges[0])):
        ac = {axis: A(not np.isnan(ranges[a][c]), None if np.isnan(ranges[a][c]) else float(ranges[a][c]))
              for a, axis in enumerate(AXES)}
        cfgs.append(tv.ObjectConfig(f"o{c}", ac["yaw"], ac["pitch"], ac["roll"], False, False, None))
    return tv.ObjectConfigSet(cfgs)


def _case(name):
    """Host inputs of a case, made once: conditioned bins and normal offsets [B, H, W, 4] per present axis,
    hand-made records (the flat index in column 7, everything else a pattern the kernel must not read) and
    planted heatmap / size / offset for the API-level runs."""
    if name in _CASES:
        return _CASES[name]
    c = dict(SMALL if name == "small" else WIDE)
    B, C, H, W, K = (c[k] for k in "BCHWK")
    rng = np.random.default_rng(7 if name == "small" else 8)
    heads = {}
    for axis in AXES:
        if axis in c["absent"]:
            continue
        bins = ref.conditioned_bins(rng, (B, H, W))
        ref.assert_conditioned(bins)
        heads[axis] = (bins, rng.normal(0.0, 1.0, (B, H, W, 4)).astype(np.float32))
    c["heads"] = heads
    records = np.full((B, K, 10), 12345.0, np.float32)
    records[..., 7] = np.stack([rng.permutation(C * H * W)[:K] for _ in range(B)])
    if name == "small":  # image 0's four live rows: every label, cells with y != x
        records[0, :4, 7] = [0 * H * W + 3 * W + 5, 1 * H * W + 4 * W + 0, 2 * H * W + 0 * W + 6, 0 * H * W + 1 * W + 2]
    c["records"], c["counts_np"] = records, np.array(c["counts"], np.int32)
    # planted peaks for the API level: distinct logits 0.25 apart on a -8 floor, no two within a 3x3
    # window of one channel (cells of a 2-strided grid), image b keeps counts[b] of them above 0 (score 0.5)
    heat = np.full((B, C, H, W), -8.0, np.float32)
    cells = [(ch, y, x) for ch in range(C) for y in range(0, H, 2) for x in range(0, W, 2)]
    for b in range(B):
        pick = rng.permutation(len(cells))
        n_pos = c["planted"][b]
        assert n_pos <= len(cells)
        if name == "small" and n_pos:  # the strongest peaks: one of each label
            first = [cells.index((ch, 2, 4 - 2 * ch)) for ch in range(C)]
            pick = first + [j for j in pick if j not in first]
        for r, j in enumerate(pick[:n_pos]):
            heat[(b,) + cells[j]] = 0.5 + 0.25 * (n_pos - r)
    c["heat"] = heat
    c["size"] = rng.uniform(0.05, 0.4, (B, H, W, 2)).astype(np.float32)
    c["offset"] = rng.uniform(0.0, 1.0, (B, H, W, 2)).astype(np.float32)
    _CASES[name] = c
    return c


def _prediction(c, form):
    """The case as a device Prediction. form "nhwc": every head a channel slice of one NHWC tensor with an
    odd channel count (so no slice is aligned or dense); "nchw": NCHW tensors permuted to NHWC."""
    from tauv_vision_amd.centernet import Prediction
    B, C, H, W = (c[k] for k in "BCHW")
    f = {k: None for k in Prediction.__dataclass_fields__}
    if form == "nhwc":
        parts = [("heatmap", c["heat"].transpose(0, 2, 3, 1)), ("size", c["size"]), ("offset", c["offset"])]
        for axis, (b, o) in c["heads"].items():
            parts += [(axis + "_bin", b), (axis + "_offset", o)]
        width = sum(p.shape[3] for _, p in parts)
        big = torch.full((B, H, W, width + 1 + width % 2), 777.0, device=DEV)
        at = 1
        for name, p in parts:
            view = big[..., at:at + p.shape[3]]
            view.copy_(torch.from_numpy(np.ascontiguousarray(p)))
            f[name] = view.permute(0, 3, 1, 2) if name == "heatmap" else view
            at += p.shape[3]
        assert not f["size"].is_contiguous()
    else:
        f["heatmap"] = torch.from_numpy(c["heat"]).to(DEV)
        f["size"], f["offset"] = torch.from_numpy(c["size"]).to(DEV), torch.from_numpy(c["offset"]).to(DEV)
        for axis, (b, o) in c["heads"].items():
            for part, a in (("bin", b), ("offset", o)):
                nchw = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).to(DEV)
                f[f"{axis}_{part}"] = nchw.permute(0, 2, 3, 1)
                assert f[f"{axis}_{part}"].stride(3) == c["H"] * c["W"]
    return Prediction(**f)


def _head_list(c):
    return [c["heads"].get(axis) for axis in AXES]


def _model_config(c):
    import tauv_vision_amd as tv
    return tv.ModelConfig([1], [1], 4 * c["H"], 4 * c["W"], 2, pi / 3)


@pytest.mark.parametrize("form", ["nhwc", "nchw"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_kernel_on_hand_made_records(name, form):
    import tauv_vision_amd as tv
    c = _case(name)
    B, H, W, K = c["B"], c["H"], c["W"], c["K"]
    dec = tv.DeviceAngleDecoder(B, K, _config(c["ranges"]), DEV)
    assert np.array_equal(dec.theta_range.cpu().numpy(), np.array(c["ranges"], np.float32), equal_nan=True)
    dec.angles.fill_(555.0)  # every element is written by every call
    records, counts = torch.from_numpy(c["records"]).to(DEV), torch.from_numpy(c["counts_np"]).to(DEV)
    got = dec(records, counts, _prediction(c, form)).cpu().numpy()
    out32, out64, period = ref.expected_angles(c["records"], c["counts_np"], _head_list(c), c["ranges"], H, W)
    live = np.arange(K)[None, :] < c["counts_np"][:, None]
    assert np.isnan(got[~live]).all(), "rows past the count must be NaN"
    if name == "small":
        assert np.isnan(got[..., 1]).all(), "the absent pitch head must give NaN"
        lab = c["records"][..., 7].astype(int) // (H * W)
        assert (lab[live] == 2).any() and (lab[live] == 1).any() and (lab[live] == 0).any()
        assert np.isnan(got[live & (lab == 2)]).all() and np.isnan(got[live & (lab == 1)][:, 0]).all()
        assert not np.isnan(got[live & (lab == 0)][:, [0, 2]]).any()
    ref.check_angles(got, out32, out64, period, f"kernel, {name}, {form}")


@pytest.mark.parametrize("form", ["nhwc", "nchw"])
@pytest.mark.parametrize("name", ["small", "wide"])
def test_decode_oriented_on_planted_peaks(name, form):
    import tauv_vision_amd as tv
    c = _case(name)
    oc, mc, pred = _config(c["ranges"]), _model_config(c), _prediction(c, form)
    records, counts, angles = tv.decode_oriented_records(pred, mc, oc, c["K"], 0.5)
    assert counts.tolist() == list(c["planted"])
    plain_records, plain_counts = tv.decode_records(pred, mc, c["K"], 0.5)
    assert np.array_equal(records, plain_records, equal_nan=True) and np.array_equal(counts, plain_counts)
    out32, out64, period = ref.expected_angles(records, counts, _head_list(c), c["ranges"], c["H"], c["W"])
    ref.check_angles(angles, out32, out64, period, f"decode_oriented_records, {name}, {form}")
    # the detection lists: decode()'s fields, plus the angles as floats / None
    dets, plain = tv.decode_oriented(pred, mc, oc, c["K"], 0.5), tv.decode(pred, mc, c["K"], 0.5)
    assert [len(d) for d in dets] == list(c["planted"]) == [len(d) for d in plain]
    for b, (db, pb) in enumerate(zip(dets, plain)):
        for i, (d, p) in enumerate(zip(db, pb)):
            assert (int(d.label), float(d.score), d.y, d.x, d.h, d.w, d.depth) == \
                   (int(p.label), float(p.score), p.y, p.x, p.h, p.w, p.depth)
            assert (p.roll, p.pitch, p.yaw) == (None, None, None)
            for a, axis in enumerate(AXES):
                v = getattr(d, axis)
                if np.isnan(angles[b, i, a]):
                    assert v is None
                else:
                    assert isinstance(v, float) and v == float(angles[b, i, a])
    if name == "small":
        assert [int(d.label) for d in dets[0][:3]] == [0, 1, 2] and all(d.pitch is None for d in dets[0])
        assert [d.yaw is None for d in dets[0][:3]] == [False, False, True]
        assert [d.roll is None for d in dets[0][:3]] == [False, True, True]


def test_saturated_scores_choose_bin_0_on_the_device():
    """Bins (-15, 15, -20, 20): both fp32 scores are exactly 1, so bin 0 is decoded (a comparison of the logit
    differences would take bin 1). And one ulp apart the other way: (-20, 20, -15, 15) is bin 0 as well."""
    import tauv_vision_amd as tv
    from tauv_vision_amd.centernet import Prediction
    B, C, H, W, K = 1, 1, 2, 3, 2
    bins = torch.zeros((B, H, W, 4))
    bins[0, 1, 2] = torch.tensor([-15.0, 15.0, -20.0, 20.0])
    bins[0, 0, 1] = torch.tensor([-20.0, 20.0, -15.0, 15.0])
    off = torch.tensor([np.sin(0.3), np.cos(0.3), np.sin(1.1), np.cos(1.1)], dtype=torch.float32).expand(B, H, W, 4)
    f = {k: None for k in Prediction.__dataclass_fields__}
    f.update(heatmap=torch.zeros((B, C, H, W), device=DEV), yaw_bin=bins.to(DEV), yaw_offset=off.contiguous().to(DEV))
    records = np.zeros((B, K, 10), np.float32)
    records[0, :, 7] = (1 * W + 2, 0 * W + 1)
    dec = tv.DeviceAngleDecoder(B, K, _config([[np.nan], [np.nan], [2 * pi]]), DEV)
    got = dec(torch.from_numpy(records).to(DEV), torch.tensor([K], dtype=torch.int32, device=DEV),
              Prediction(**f)).cpu().numpy()
    assert np.isnan(got[..., :2]).all()
    assert np.abs(got[0, :, 2] - (pi / 2 + 0.3)).max() <= 2.0 ** -20, got[0, :, 2]


def test_graph_replay_equals_eager():
    """tv_decode + tv_decode_angles captured in one graph: replayed over clobbered outputs, the packed
    buffer (records, counts, angles) is bit-equal to the eager run."""
    import tauv_vision_amd as tv
    c = _case("wide")
    B, C, H, W, K = (c[k] for k in "BCHWK")
    mc, pred = _model_config(c), _prediction(c, "nhwc")
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        dec = tv.DeviceDecoder(B, C, H, W, K, DEV, angles=True)
        ang = tv.DeviceAngleDecoder(B, K, _config(c["ranges"]), DEV, out=dec.angles)
        assert dec.packed.numel() == (B * K * 10 + B + B * K * 3) * 4

        def step():
            dec(pred.heatmap, pred.size, pred.offset, None, 0, mc.downsample_ratio, mc.in_h, mc.in_w, 0.5)
            ang(dec.records, dec.counts, pred)

        step()
        s.synchronize()
        eager = dec.packed.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            step()
        for _ in range(2):
            dec.packed.fill_(0x5A)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(dec.packed, eager)
    torch.cuda.current_stream(DEV).wait_stream(s)
    assert dec.counts.tolist() == list(c["planted"]) and not torch.isnan(dec.angles[0, :c["planted"][0]]).any()


def test_every_refusal_and_the_empty_batch():
    from tauv_vision_amd import _lib
    B, C, H, W, K = 2, 3, 5, 7, 6
    buf = torch.zeros(B * H * W * 4 + B * K * 10, dtype=torch.float32, device=DEV)
    out = torch.full((B, K, 3), 7.0, device=DEV)
    p, o, null = ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(out.data_ptr()), None
    st = (ctypes.c_int64 * 4)(H * W * 4, W * 4, 4, 1)
    ok = dict(records=p, rec_stride=10, counts=p, heads=[p, st] * 6, theta=p, B=B, C=C, H=H, W=W, K=K, angles=o)

    def call(**change):
        a = dict(ok, **change)
        return _lib.lib().tv_decode_angles(a["records"], a["rec_stride"], a["counts"], *a["heads"], a["theta"], a["B"],
                                           a["C"], a["H"], a["W"], a["K"], a["angles"], _lib.stream_of(DEV))

    bin_only, offset_only = [p, st, null, null] + [p, st] * 4, [p, st] * 2 + [null, null, p, st] + [p, st] * 2
    refused = [dict(records=null), dict(counts=null), dict(theta=null), dict(angles=null), dict(rec_stride=7),
               dict(heads=bin_only), dict(heads=offset_only), dict(heads=[p, null] + [p, st] * 5), dict(C=0), dict(H=0),
               dict(W=-1), dict(K=0), dict(B=-1), dict(C=4096, H=64, W=64)]
    for change in refused:
        rc = call(**change)
        assert rc == _lib.TV_EINVAL, change
        with pytest.raises(ValueError, match="decode_angles"):
            _lib.check(rc, "decode_angles")
    assert call(C=4095, H=64, W=64, B=0) == _lib.TV_OK  # just below 2^24
    assert call(B=0) == _lib.TV_OK
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused or empty call wrote its output"
    # all heads absent: allowed, everything NaN (records and counts are zeros: count 0)
    assert call(heads=[null, null] * 6) == _lib.TV_OK
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_decoder_refusals():
    import tauv_vision_amd as tv
    c = _case("small")
    oc, pred = _config(c["ranges"]), _prediction(c, "nchw")
    dec = tv.DeviceAngleDecoder(c["B"], c["K"], oc, DEV)
    dec.angles.fill_(3.0)
    records, counts = torch.from_numpy(c["records"]).to(DEV), torch.from_numpy(c["counts_np"]).to(DEV)
    with pytest.raises(ValueError, match="records must be"):
        dec(records.cpu(), counts, pred)
    with pytest.raises(ValueError, match="shapes"):
        dec(records[:, :-1].contiguous(), counts, pred)
    wrong = _prediction(c, "nchw")
    wrong.yaw_offset = wrong.yaw_offset[:, :-1]
    with pytest.raises(ValueError, match="yaw_offset"):
        dec(records, counts, wrong)
    one_label = tv.DeviceAngleDecoder(c["B"], c["K"], _config([[pi], [pi], [pi]]), DEV)
    with pytest.raises(ValueError, match="heatmap must be"):
        one_label(records, counts, pred)
    with pytest.raises(ValueError, match="labels"):
        tv.decode_oriented_records(pred, _model_config(c), _config([[pi], [pi], [pi]]), c["K"], 0.5)
    torch.cuda.synchronize()
    assert (dec.angles == 3.0).all(), "a refused call launched"


def test_detect_with_angles_equals_decode_oriented_of_the_forward():
    import tauv_vision_amd as tv
    from recipe import seeded_u8_frames
    from tauv_vision_amd.weights import seeded_state_dict
    heights, channels, ds = [2] * 5, [16] * 6, 2
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([
        tv.ObjectConfig("square", A(True, pi / 2), A(False, None), A(False, None), False, False, None),
        tv.ObjectConfig("free", A(True, 2 * pi), A(False, None), A(True, pi), False, False, None)])
    model = tv.Centernet(tv.DLABackbone(heights, channels, ds), oc, precision="fp32")
    model.load_state_dict(seeded_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()]))
    model = model.to(DEV).eval()
    mc = tv.ModelConfig(heights, channels, 96, 128, ds, pi / 3)
    frames = seeded_u8_frames(2, 96, 128, seed=3)
    pred = model.forward_frames(frames, (96, 128))
    assert pred.yaw_bin is not None and pred.roll_bin is not None and pred.pitch_bin is None
    want = tv.decode_oriented(pred, mc, oc, 12, 0.0)
    got = model.detect(frames, mc, 12, 0.0, angles=True)
    plain = model.detect(frames, mc, 12, 0.0)
    assert [len(d) for d in got] == [12, 12] == [len(d) for d in plain]
    fields = lambda d: (int(d.label), float(d.score), d.y, d.x, d.h, d.w, d.depth, d.roll, d.pitch, d.yaw)
    for gb, wb, pb in zip(got, want, plain):
        for g, w, p in zip(gb, wb, pb):
            assert fields(g) == fields(w)
            assert fields(p)[:7] == fields(g)[:7] and (p.roll, p.pitch, p.yaw) == (None, None, None)
            assert g.pitch is None and isinstance(g.yaw, float) and 0 <= g.yaw <= (pi / 2, 2 * pi)[int(g.label)] * 1.000001
            assert (g.roll is None) == (int(g.label) == 0)
