"""YOLACT neck + head on the GPU (TV_ARCH_YOLACT_HEAD / TV_ARCH_YOLACT_FPN: csrc/planner_yolact_head.cpp,
csrc/yolact_head.hip, the engine's several inputs and outputs) against the reference's goldens
(tests/golden/gen_golden_yolact_head.py) and the torch restatement pinned to them
(tests/yolact_head_ref.py, tests/test_yolact_head_cpu.py).

Bars: bilinear_add in fp32 within 1e-6 of F.interpolate + add (fp16 / bf16: one rounding of the
interpolated value and one of the sum); fp32 and fp32x3 within 1e-4 * max(1, |ref|max) per tensor, the
project's fp32 bar; fp16 / bf16 within 3x the drift measured on MI355X
(profiles/yolact_head/parity_yolact_head.json); the row order checked element by element."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolact_head_ref as yr
from helpers import golden, record_measurement
from recipe_yolact_head import HEAD_CASES, head_case, head_level_sizes, head_sample_index
from test_yolact_head_cpu import case_config, case_inputs

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "fp32x3", "fp16", "bf16"]
NAMES = [c["name"] for c in HEAD_CASES]
# fp32 / fp32x3: the standing fp32 bar. fp16 / bf16: 3x the largest drift of any tensor of any case
# measured on MI355X, relative to max(1, |ref|max) (profiles/yolact_head/parity_yolact_head.json:
# the worst of both is case D's tanh'd mask coefficients, fp16 5.24e-3, bf16 3.71e-2 — five levels of
# low-precision activations under a 2304-term sum; the fp32 paths measure 4.7e-6 / 7.4e-6 there)
TOL = {"fp32": 1e-4, "fp32x3": 1e-4, "fp16": 3 * 5.24e-3, "bf16": 3 * 3.71e-2}
_DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _check(key, got, ref, precision):
    """max |got - ref| against the precision's bound, relative to max(1, |ref|max); recorded first."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{key}: {got.shape} vs {ref.shape}"
    err, scale = float(np.abs(got - ref).max()), max(1.0, float(np.abs(ref).max()))
    record_measurement(f"yolact_head/{key}/{precision}", {"max_abs_err": err, "ref_absmax": scale, "rel": err / scale})
    print(f"yolact_head/{key}/{precision}: err {err:.3e} scale {scale:.3f} rel {err / scale:.3e}")
    assert np.isfinite(got).all(), f"{key} {precision}: non-finite values"
    assert err <= TOL[precision] * scale, f"{key} {precision}: {err} > {TOL[precision]} * {scale}"


# ---- bilinear_add alone ----

@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("src,dst", [((3, 3), (5, 6)), ((5, 6), (9, 11)), ((1, 1), (2, 2)), ((4, 4), (8, 8)),
                                     ((18, 18), (35, 35))])
def test_bilinear_add_matches_interpolate(src, dst, C, precision):
    from tauv_vision_amd import _lib
    dt, B = _DT[precision], 2
    g = torch.Generator().manual_seed(7 + C + dst[0])
    # values in (-1, 1): the interpolated value stays within (-1, 1), the sum within (-2, 2)
    x = (torch.rand((B, *src, C), generator=g) * 2 - 1).to(dt)
    y = (torch.rand((B, *dst, C), generator=g) * 2 - 1).to(dt)
    up = F.interpolate(x.float().permute(0, 3, 1, 2), dst, mode="bilinear").permute(0, 2, 3, 1)
    ref = y.float() + up
    pad = 16 // x.element_size()  # one more vector per pixel, which the kernel must leave alone
    d = torch.full((B, *dst, C + pad), float("nan"), dtype=dt)
    d[..., :C] = y
    d = d.cuda()
    _lib.check(_lib.lib().tv_diag_bilinear_add(ctypes.c_void_p(x.cuda().data_ptr()), B, src[0], src[1], C,
                                               ctypes.c_void_p(d.data_ptr()), dst[0], dst[1], C + pad, C,
                                               _lib.DTYPES[precision], _lib.stream_of(d.device)), "bilinear_add")
    got = d.cpu().float()
    assert torch.isnan(got[..., C:]).all(), "wrote past the C channels"
    err = float((got[..., :C] - ref).abs().max())
    # fp16 / bf16: half an ulp of the interpolated value (|v| < 1) + half an ulp of the sum (|s| < 2)
    bound = {"fp32": 1e-6, "fp16": 2.0 ** -12 + 2.0 ** -11, "bf16": 2.0 ** -9 + 2.0 ** -8}[precision]
    print(f"bilinear_add {src}->{dst} C={C} {precision}: err {err:.3e}")
    assert err <= bound, f"{src}->{dst} C={C} {precision}: {err}"


def test_bilinear_add_refuses_partial_vectors():
    from tauv_vision_amd import _lib
    x, d = torch.zeros(1, 2, 2, 32).cuda(), torch.zeros(1, 4, 4, 32).cuda()
    for C, sl, dl in ((30, 32, 32), (32, 34, 32), (32, 32, 28)):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().tv_diag_bilinear_add(ctypes.c_void_p(x.data_ptr()), 1, 2, 2, sl,
                                                       ctypes.c_void_p(d.data_ptr()), 4, 4, dl, C, 0,
                                                       _lib.stream_of(d.device)), "bilinear_add")


# ---- conv_burst on the K sizes the neck brings ----

# (B, Ho, Wo, [(C, kernel, stride)], N, act): layers whose K quarter per wave (k-steps / 4) is shorter
# than the compiled instance's (quarters of 2 on the 4-step instance: the 128-channel lateral conv at
# 69x69; quarters of 10 on the 12-step one). Before the quarter bounded each wave's k-steps, waves
# summed their neighbours' k-steps too.
BURST_SHAPES = [
    (1, 69, 69, [(128, 1, 1)], 256, 0),
    (2, 9, 9, [(128, 1, 1)], 40, 1),
    (2, 5, 5, [(256, 1, 1), (256, 1, 1), (128, 1, 1)], 64, 2),
]


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("B,Ho,Wo,segspec,N,act", BURST_SHAPES)
def test_burst_short_k_quarters_vs_torch(B, Ho, Wo, segspec, N, act, precision):
    import test_gpu_conv_burst as tb
    tb.test_burst_single_layer_vs_torch(B, Ho, Wo, segspec, N, act, precision)


# ---- the neck and the head against the goldens ----

def _head(c, precision, sd=None):
    from tauv_vision_amd.yolact import YolactHead
    head = YolactHead(c["depths"], case_config(c), precision=precision)
    if sd is not None:
        head.load_state_dict(sd)
    return head


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_feature_pyramid_matches_reference(name, precision):
    from tauv_vision_amd.yolact import FeaturePyramid
    c, g = head_case(name), golden(name)
    sd, maps = case_inputs(c)
    p = "_feature_pyramid."
    fpn = FeaturePyramid(c["depths"], case_config(c), precision=precision)
    fpn.load_state_dict({k[len(p):]: v for k, v in sd.items() if k.startswith(p)})
    out = fpn([m.cuda() for m in maps])
    assert [tuple(o.shape[2:]) for o in out] == head_level_sizes(c)
    for i, o in enumerate(out):
        assert tuple(o.shape[:2]) == (c["batch"], c["F"])
        o = o.cpu()
        if f"fpn{i}" in g:
            _check(f"{name}/fpn{i}", o.numpy(), g[f"fpn{i}"], precision)
        # per-channel sums over every value: a systematic bias grows like n
        n = o.shape[0] * o.shape[2] * o.shape[3]
        scale = max(1.0, float(o.abs().max()))
        np.testing.assert_allclose(o.double().sum(dim=(0, 2, 3)).numpy(), g[f"fpn_chan_sum{i}"],
                                   rtol=TOL[precision], atol=4 * TOL[precision] * scale * n ** 0.5)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", NAMES)
def test_yolact_head_matches_reference(name, precision):
    c, g = head_case(name), golden(name)
    sd, maps = case_inputs(c)
    head = _head(c, precision, sd)
    cls, enc, coef, anchor, proto = head([m.cuda() for m in maps])
    for t in (cls, enc, coef):
        assert t.is_contiguous() and t.dtype == torch.float32
    np.testing.assert_array_equal(anchor.cpu().numpy(), g["anchor"])
    _check(f"{name}/cls", cls.cpu().numpy(), g["cls"], precision)
    _check(f"{name}/enc", enc.cpu().numpy(), g["enc"], precision)
    _check(f"{name}/coef", coef.cpu().numpy(), g["coef"], precision)
    assert tuple(proto.shape) == tuple(g["proto_shape"])
    proto = proto.cpu().contiguous()
    if c["full"]:
        _check(f"{name}/proto", proto.numpy(), g["proto"], precision)
    else:
        _check(f"{name}/proto", proto.reshape(-1)[head_sample_index(c)].numpy(), g["proto_sample"], precision)
    n = proto.shape[0] * proto.shape[2] * proto.shape[3]
    scale = max(1.0, float(proto.abs().max()))
    np.testing.assert_allclose(proto.double().sum(dim=(0, 2, 3)).numpy(), g["proto_chan_sum"],
                               rtol=TOL[precision], atol=4 * TOL[precision] * scale * n ** 0.5)


def test_row_order_is_pixel_major_ratio_inner():
    """Case B (three aspect ratios, unstacked heads): element [b, off_l + (y W + x) n_ar + a, j] of each
    output is channel a * width + j at pixel (y, x) of the level's final conv — a ratio-major layout
    or a wrong level offset moves values by whole rows, far beyond any tolerance."""
    c = head_case("yolact_head_b")
    sd, maps = case_inputs(c)
    outs = _head(c, "fp32", sd)([m.cuda() for m in maps])
    got = [outs[0].cpu(), outs[1].cpu(), outs[2].cpu()]
    nar, widths = len(c["ars"]), (c["C"] + 1, 4, c["k"])
    with torch.no_grad():
        fpn = yr.feature_pyramid(sd, maps)
        off = 0
        for f in fpn:
            raw = yr.prediction_head_raw(sd, f)
            H, W = f.shape[2:]
            for j, (r, wd) in enumerate(zip(raw, widths)):
                assert r.shape[1] == nar * wd
                if j == 2:
                    r = torch.tanh(r)
                # [B, n_ar, width, H, W] -> rows (y, x, a), columns j
                want = r.reshape(1, nar, wd, H, W).permute(0, 3, 4, 1, 2).reshape(1, H * W * nar, wd)
                tol = 1e-4 * max(1.0, float(want.abs().max()))
                block = got[j][:, off:off + H * W * nar]
                assert float((block - want).abs().max()) <= tol, f"output {j}, level {H}x{W}"
                # the ratio-major order must NOT match (the check has teeth)
                wrong = r.reshape(1, nar, wd, H * W).permute(0, 1, 3, 2).reshape(1, H * W * nar, wd)
                assert H * W == 1 or float((block - wrong).abs().max()) > 100 * tol
            off += H * W * nar
    assert off == outs[0].shape[1]


# ---- batches, slices, graphs ----

def _rand_maps(c, B, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((B, d, h, w), generator=g).cuda() for d, (h, w) in zip(c["depths"], c["sizes"])]


def test_batch_slices_match_single_frames():
    """B = 17 runs as two concurrent slices (9 + 8 frames), each pointer advanced by its own frame
    size. Frames 0, 8 and 16 equal their single-frame results within fp16 rounding (the bound of
    test_gpu_protonet_batch_consistency: the kernel choice and so the order of the K sums may depend
    on the batch), and a repeat is bit-identical."""
    c = head_case("yolact_head_a")
    sd, _ = case_inputs(c)
    head = _head(c, "fp16", sd)
    maps = _rand_maps(c, 17, 11)
    outs = [o.clone() for o in head(maps)]
    assert head.engine(maps[0].device, c["sizes"]).slices(17) == [9, 8]
    for a, b in zip(head(maps), outs):
        assert torch.equal(a, b)
    for i in (0, 8, 16):
        one = head([m[i:i + 1] for m in maps])
        for j in (0, 1, 2, 4):
            scale = max(1.0, float(outs[j].abs().max()))
            np.testing.assert_allclose(one[j].cpu().numpy(), outs[j][i:i + 1].cpu().numpy(), rtol=0, atol=1e-3 * scale)


def test_graph_replay_of_out_form_is_bit_equal():
    c = head_case("yolact_head_a")
    sd, _ = case_inputs(c)
    head = _head(c, "fp16", sd)
    dev = torch.device("cuda", 0)
    B = 3
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        maps = _rand_maps(c, B, 12)
        first = head(maps)
        out = [torch.empty_like(first[0]), torch.empty_like(first[1]), torch.empty_like(first[2]),
               torch.empty((B, 4 * c["sizes"][0][0], 4 * c["sizes"][0][1], (c["k"] + 3) // 4 * 4), device=dev)]
        res = head(maps, out=out)  # the eager step on the capture stream: its workspaces exist before the capture
        assert res[0].data_ptr() == out[0].data_ptr() and res[4].data_ptr() == out[3].data_ptr()
        s.synchronize()
        eager = [o.clone() for o in out]
        for a, b in zip((first[0], first[1], first[2]), eager):
            assert torch.equal(a, b)
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        head(maps, out=out)
    for _ in range(2):
        for o in out:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(out, eager):
            assert torch.equal(o, e), "replayed outputs differ from the eager step"


def test_load_state_dict_rebuilds_engine():
    from tauv_vision_amd.yolact import yolact_head_state_dict
    c = head_case("yolact_head_c")
    sd, maps = case_inputs(c)
    g = golden(c["name"])
    maps = [m.cuda() for m in maps]
    head = _head(c, "fp32")          # its own seeded weights, not the case's
    before = head(maps)[0].clone()
    eng = head.engine(maps[0].device, c["sizes"])
    full = dict(sd)
    full["_backbone._feature_extractor.conv1.weight"] = torch.zeros(4, 3, 7, 7)
    head.load_state_dict(yolact_head_state_dict(full))
    assert head.engine(maps[0].device, c["sizes"]) is not eng, "a reload must invalidate the engine"
    after = head(maps)[0]
    assert float((after - before).abs().max()) > 1e-2
    _check("reload/cls", after.cpu().numpy(), g["cls"], "fp32")
    with pytest.raises(RuntimeError, match="_mask_coeff_layer.weight"):
        head.load_state_dict({k: v for k, v in sd.items() if k != "_prediction_head._mask_coeff_layer.weight"})


def test_refusals_before_any_launch():
    from tauv_vision_amd import _lib
    c = head_case("yolact_head_c")
    head = _head(c, "fp32")
    maps = _rand_maps(c, 2, 13)
    with pytest.raises(ValueError, match="expected 3 backbone maps"):
        head(maps[:2])
    with pytest.raises(ValueError, match="backbone map 1"):
        head([maps[0], maps[1][:, :16], maps[2]])               # a wrong depth
    with pytest.raises(ValueError, match="on cpu"):
        head([maps[0], maps[1].cpu(), maps[2]])                 # a map on another device
    good = head(maps)
    A, k = good[0].shape[1], c["k"]
    h, w = c["sizes"][0]
    ok = lambda: [torch.empty(2, A, c["C"] + 1).cuda(), torch.empty(2, A, 4).cuda(), torch.empty(2, A, k).cuda(),
                  torch.empty(2, 4 * h, 4 * w, (k + 3) // 4 * 4).cuda()]
    for i, bad in ((0, torch.empty(2, A + 1, c["C"] + 1).cuda()), (1, torch.empty(2, A, 4, dtype=torch.float16).cuda()),
                   (2, torch.empty(2, k, A).cuda().transpose(1, 2)), (3, torch.empty(2, 4 * h, 4 * w, 8)),
                   (0, torch.empty(1, A, c["C"] + 1).cuda())):
        out = ok()
        out[i] = bad
        with pytest.raises(ValueError, match="out"):
            head(maps, out=out)
    with pytest.raises(ValueError, match="4 tensors"):
        head(maps, out=ok()[:3])
    res = head(maps, out=ok())
    for a, b in zip(res[:3], good[:3]):
        assert torch.equal(a, b)
    # the single-pointer C entry points refuse the multi-input archs
    eng = head.engine(maps[0].device, c["sizes"])
    with pytest.raises(ValueError, match="3 input"):
        eng.forward(maps[0])
    L = _lib.lib()
    ms, fl, n = (ctypes.c_float * 64)(), (ctypes.c_double * 64)(), ctypes.c_int32()
    assert L.tv_engine_profile(eng._h, ctypes.c_void_p(maps[0].data_ptr()), 2, ctypes.c_void_p(good[0].data_ptr()),
                               _lib.stream_of(eng.device), ms, fl, 64, ctypes.byref(n)) == _lib.TV_EINVAL
    ptrs = (ctypes.c_void_p * 3)(*[m.data_ptr() for m in maps])
    outs = (ctypes.c_void_p * 4)(*[o.data_ptr() for o in ok()])
    assert L.tv_engine_forward_multi(eng._h, ptrs, 2, outs, 4, 2, _lib.stream_of(eng.device)) == _lib.TV_EINVAL
    assert L.tv_engine_forward_multi(eng._h, ptrs, 3, outs, 3, 2, _lib.stream_of(eng.device)) == _lib.TV_EINVAL
    torch.cuda.synchronize()


def test_profile_multi_lists_the_new_kernels():
    c = head_case("yolact_head_a")
    sd, maps = case_inputs(c)
    head = _head(c, "fp16", sd)
    maps = [m.cuda() for m in maps]
    want = head(maps)
    eng = head.engine(maps[0].device, c["sizes"])
    outs = [torch.empty_like(want[0]), torch.empty_like(want[1]), torch.empty_like(want[2]),
            torch.empty((c["batch"], 4 * c["sizes"][0][0], 4 * c["sizes"][0][1], 8), device=maps[0].device)]
    rows = eng.profile_multi(maps, outs)
    kernels = [r[3] for r in rows]
    assert sum(k.startswith("tv::yh::bilinear_add<") for k in kernels) == 2
    assert kernels.count("tv::yh::head_scatter") == 5
    assert sum(k.startswith("tv::nchw_to_nhwc<") for k in kernels) == 3
    for a, b in zip(outs[:3], want[:3]):  # one op per launch, the same kernels: the same result
        assert torch.equal(a, b)


# ---- end to end: the head's outputs through the raw-pointer consumers ----

def test_end_to_end_nms_indices_and_masks():
    """YolactHead -> box_decode -> nms(100, 0.5, 0.05) -> assemble_mask in fp32 on the margin-checked
    case (tests/golden/gen_golden_yolact_head.py gen_e2e: consecutive confidences, the confidence
    threshold and every pairwise IoU the decision reads are more than 1e-3 from a tie, so the fp32
    path's ~1e-6 cannot flip a decision): exactly the reference's indices, masks within 1e-4."""
    from recipe_yolact_head import E2E_NMS
    from test_yolact_head_cpu import e2e_case
    from tauv_vision_amd.yolact import assemble_mask, box_decode, nms
    c = e2e_case()
    g = golden(c["name"])
    sd, maps = case_inputs(c)
    cfg = case_config(c)
    cls, enc, coef, anchor, proto = _head(c, "fp32", sd)([m.cuda() for m in maps])
    box = box_decode(enc, anchor, cfg)
    _check("e2e/box", box.cpu().numpy(), g["box"], "fp32")
    det = nms(cls, box, *E2E_NMS)
    np.testing.assert_array_equal(det.cpu().numpy(), g["det"])
    mask = assemble_mask(proto[0], coef[0, det], box[0, det])
    err = float(np.abs(mask.cpu().numpy() - g["mask"]).max())
    print(f"e2e mask err {err:.3e}")
    assert err <= 1e-4, err


def test_set_precision_is_the_heads_one_switch():
    """Only YolactHead's precision selects the engine; a sub-module's own precision does not."""
    c = head_case("yolact_head_c")
    sd, maps = case_inputs(c)
    g = golden(c["name"])
    maps = [m.cuda() for m in maps]
    head = _head(c, "fp32", sd)
    exact = head(maps)[0].clone()
    head._feature_pyramid.precision = "bf16"          # a holder's field: no effect on the head
    assert torch.equal(head(maps)[0], exact)
    head.set_precision("fp16")
    assert head._feature_pyramid.precision == head._masknet.precision == "fp16"
    low = head(maps)[0]
    assert not torch.equal(low, exact)
    _check("set_precision/cls", low.cpu().numpy(), g["cls"], "fp16")
    with pytest.raises(ValueError):
        head.set_precision("fp8")
