"""The YOLACT instance masks at frame size (csrc/yolact_frame.hip: packed bits, areas, overlay) against
tests/frame_masks_ref.py, the host restatement of evaluate_batch.py:98-102,136-139, yolact_node.py:135,143,184
and utils/plot.py:148-152, which tests/test_frame_masks_ref_cpu.py pins to the reference's own fixture.

The inputs are synthetic masks (frame_masks_ref.synthetic_masks: sigmoid of a bicubically enlarged 5 x 6
random field, times a box crop), so the kernel and the reference read the same fp32 values.

Nearest: no arithmetic on the values, so the bits equal F.interpolate(m, (H, W)) > 0.5 everywhere.
Bilinear: v64 is float64 F.interpolate and v32 the fp32 one, both on the CPU; e_ref = max |v32 - v64|,
band = max(4 e_ref, 2^-20) (the rule of the loss tests), computed here from the reference alone and
printed. The bits must equal v64 > 0.5 wherever |v64 - 0.5| > band, and at most 0.1 % of a case's pixels
may lie inside the band (else the case is vacuous). The overlay is integer arithmetic on the kernel's own
bits: exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import frame_masks_ref as ref
import tauv_vision_amd as tv
from tauv_vision_amd.yolact import DeviceFrameMasks, FrameMasks, frame_masks, unpack_frame_masks

pytestmark = pytest.mark.gpu

# (mh, mw, H, W, n)
SHAPES = {
    "18x22_to_45x70": (18, 22, 45, 70, 6),     # W neither a multiple of 32 nor of 64
    "19x23_to_64x65": (19, 23, 64, 65, 6),     # one pixel into a second wave
    "16x36_to_33x127": (16, 36, 33, 127, 6),
    "37x53_to_36x50": (37, 53, 36, 50, 6),     # down-scaling, W < 64
    "23x40_to_90x160": (23, 40, 90, 160, 6),
    "18x22_to_45x70_n70": (18, 22, 45, 70, 70),  # more detections than a wave has lanes
}
COUNTS = {6: ([6, 0], [3, 6]), 70: ([70, 0], [65, 70])}
B = 2


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of a shape and everything computed from the reference alone, once for all tests."""
    mh, mw, H, W, n = SHAPES[name]
    raw, box = ref.synthetic_masks(B, n, mh, mw, seed=len(name) * 100 + n)
    # planted for the nearest mode, which copies values: some exactly at the threshold (not selected: the
    # test is `>`), and a detection that is nowhere above it. (Bilinear takes the masks as they are: a
    # plateau of 0.5 interpolates to 0.5, inside any band.)
    planted = raw.clone()
    near = (planted > 0.5) & (planted < 0.55)
    near[0, 1] = False
    assert int(near.sum()) > 10
    planted[near] = 0.5
    planted[0, 1] = planted[0, 1].clamp(max=0.5)
    assert float(planted[0, 1].max()) == 0.5
    masks = {"nearest": planted, "bilinear": raw}
    up = {mode: ref.upsample(masks[mode], (H, W), mode) for mode in ("nearest", "bilinear")}
    v64 = ref.upsample(raw, (H, W), "bilinear", torch.float64)
    e_ref = float((up["bilinear"].double() - v64).abs().max())
    band = max(4 * e_ref, 2.0 ** -20)
    # the boxes of the detections as rows of a larger, shuffled box tensor (what BatchedNMS's det indexes)
    g = torch.Generator().manual_seed(n)
    A = n + 3
    det = torch.stack([torch.randperm(A, generator=g)[:n] for _ in range(B)]).to(torch.int64)
    box_all = torch.rand((B, A, 4), generator=g)
    for b in range(B):
        box_all[b, det[b]] = box[b]
    return dict(masks=masks, box=box_all, det=det, A=A, up=up, v64=v64, e_ref=e_ref, band=band)


def _run(c, name, counts, mode, bounded, frames=None, records=None, palette=None):
    """frame_masks into buffers pre-filled with ones; -> (FrameMasks on the host, sel bool [B, n, H, W])."""
    mh, mw, H, W, n = SHAPES[name]
    dev = _dev()
    ww = (W + 31) // 32
    out = FrameMasks(torch.full((B, n, H, ww), -1, dtype=torch.int32, device=dev).view(torch.uint32),
                     torch.ones((B, n), dtype=torch.int32, device=dev),
                     None if frames is None else torch.full((B, H, W, 3), 255, dtype=torch.uint8, device=dev))
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    fm = frame_masks(c["masks"][mode].to(dev), cnt, (H, W), mode, det=c["det"].to(dev) if bounded else None,
                     box=c["box"].to(dev) if bounded else None, frames=frames, records=records, palette=palette, out=out)
    assert fm.bits.data_ptr() == out.bits.data_ptr() and fm.area.data_ptr() == out.area.data_ptr()
    assert (fm.overlay is None) == (frames is None)
    host = FrameMasks(fm.bits.cpu(), fm.area.cpu(), None if fm.overlay is None else fm.overlay.cpu())
    return host, unpack_frame_masks(host.bits, W)


def _check_layout(host, sel, counts, W):
    """Pad bits zero, rows past the count zero, area == popcount(bits)."""
    full = unpack_frame_masks(host.bits, host.bits.shape[-1] * 32)
    assert not full[..., W:].any(), "bits at x >= W must be zero"
    assert torch.equal(full[..., :W], sel)
    for b, cb in enumerate(counts):
        assert not (host.bits[b, cb:].view(torch.int32) != 0).any(), f"rows past counts[{b}] must be zero"
        assert not host.area[b, cb:].any()
    assert torch.equal(host.area.long(), sel.flatten(2).sum(-1)), "area == popcount(bits)"


@pytest.mark.parametrize("name", list(SHAPES))
def test_nearest_is_exact(name):
    mh, mw, H, W, n = SHAPES[name]
    c = _case(name)
    for counts in COUNTS[n]:
        want = c["up"]["nearest"] > 0.5
        for b, cb in enumerate(counts):
            want[b, cb:] = False
        host, sel = _run(c, name, counts, "nearest", bounded=False)
        _check_layout(host, sel, counts, W)
        assert torch.equal(sel, want), "unpack(bits) == F.interpolate(m, (H, W)) > 0.5"
        bounded, _ = _run(c, name, counts, "nearest", bounded=True)
        assert torch.equal(bounded.bits.view(torch.int32), host.bits.view(torch.int32)), "bound_by_box changes no bit"
        assert torch.equal(bounded.area, host.area)
    # the planted values were reached, and selected nothing
    at_half = c["up"]["nearest"] == 0.5
    assert int(at_half[0, 0].sum()) + int(at_half[1].sum()) > 0
    host, sel = _run(c, name, COUNTS[n][1], "nearest", bounded=False)
    assert not (sel & at_half).any()
    assert int(host.area[0, 1]) == 0 and int(host.area[0, 0]) > 0, "a detection nowhere above 0.5 has area 0"


@pytest.mark.parametrize("name", list(SHAPES))
def test_bilinear_within_the_reference_band(name):
    mh, mw, H, W, n = SHAPES[name]
    c = _case(name)
    v64, band = c["v64"], c["band"]
    clear = (v64 - 0.5).abs() > band
    share = 1.0 - float(clear.double().mean())
    disagree = int((((c["up"]["bilinear"] > 0.5) != (v64 > 0.5)) & clear).sum())
    print(f"{name}: e_ref {c['e_ref']:.3e}, band {band:.3e}, share of pixels in the band {share:.2e}, "
          f"fp32 reference disagrees outside the band at {disagree} pixels")
    assert share <= 1e-3, "more than 0.1 % of the pixels lie within the band: the case decides nothing"
    for counts in COUNTS[n]:
        want = v64 > 0.5
        live = clear.clone()
        for b, cb in enumerate(counts):
            want[b, cb:] = False
            live[b, cb:] = True  # rows past the count are zero without any tolerance
        host, sel = _run(c, name, counts, "bilinear", bounded=False)
        _check_layout(host, sel, counts, W)
        wrong = (sel != want) & live
        assert not wrong.any(), f"{int(wrong.sum())} pixels outside the band differ from float64"
        bounded, _ = _run(c, name, counts, "bilinear", bounded=True)
        assert torch.equal(bounded.bits.view(torch.int32), host.bits.view(torch.int32)), "bound_by_box changes no bit"
        assert torch.equal(bounded.area, host.area)
    assert int(host.area.sum()) > 0


def test_a_det_entry_that_is_no_box_row_is_not_bounded():
    name = "18x22_to_45x70"
    c = dict(_case(name))
    want, _ = _run(c, name, [3, 6], "bilinear", bounded=False)
    det = c["det"].clone()
    det[0, 0], det[1, 4] = -1, c["A"]
    c["det"] = det
    got, _ = _run(c, name, [3, 6], "bilinear", bounded=True)
    assert torch.equal(got.bits.view(torch.int32), want.bits.view(torch.int32)) and torch.equal(got.area, want.area)


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("name", ["18x22_to_45x70", "19x23_to_64x65", "37x53_to_36x50", "18x22_to_45x70_n70"])
def test_overlay_is_the_restated_blend_of_the_kernels_bits(name, mode):
    mh, mw, H, W, n = SHAPES[name]
    c = _case(name)
    dev = _dev()
    g = torch.Generator().manual_seed(H * W)
    frames = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    class_id = torch.randint(0, 10, (B, n), generator=g)
    class_id[0, 0], class_id[1, 2] = 12, 10  # past the ten colours: the last one
    records = torch.rand((B, n, 8), generator=g)
    records[..., 1] = class_id.float()
    for counts in COUNTS[n]:
        for palette in (None, torch.tensor([[250, 3, 77], [0, 255, 128], [9, 9, 200]], dtype=torch.uint8)):
            host, sel = _run(c, name, counts, mode, bounded=True, frames=frames.to(dev), records=records.to(dev),
                             palette=None if palette is None else palette.to(dev))
            plain, _ = _run(c, name, counts, mode, bounded=False)
            assert torch.equal(plain.bits.view(torch.int32), host.bits.view(torch.int32)), "the overlay changes no bit"
            want = ref.blend(frames.numpy(), sel.numpy(), counts, class_id.numpy(),
                             ref.TAB10 if palette is None else palette.numpy())
            assert np.array_equal(host.overlay.numpy(), want)
        if max(counts) == n and min(counts) > 0:
            b = counts.index(n)
            assert (sel[b].sum(0) > 1).any(), "no two detections overlap: the order of the blend is not tested"
            assert not np.array_equal(want[b], frames[b].numpy())
    # an image without detections keeps its frame
    host, _ = _run(c, name, COUNTS[n][0], mode, bounded=True, frames=frames.to(dev), records=records.to(dev))
    assert torch.equal(host.overlay[1], frames[1])


def test_nearest_area_equals_the_localizers_pixel_count():
    name = "23x40_to_90x160"
    mh, mw, H, W, n = SHAPES[name]
    c = _case(name)
    dev = _dev()
    counts = [3, 6]
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    host, _ = _run(c, name, counts, "nearest", bounded=True)
    depth = torch.full((1, H, W), 1500, dtype=torch.int32).to(torch.uint16).to(dev)  # no zero depth: every mask pixel counts
    pts = tv.DeviceLocalizer(B, n, dev).masks(c["masks"]["nearest"].to(dev), cnt, c["det"].to(dev), c["box"].to(dev), depth, 100.0,
                                              100.0, 80.0, 45.0, bound_by_box=True).cpu()
    assert torch.equal(pts[..., 4].long(), host.area.long())
    assert int(host.area.sum()) > 0


def test_device_frame_masks_static_buffers():
    name = "19x23_to_64x65"
    mh, mw, H, W, n = SHAPES[name]
    c = _case(name)
    dev = _dev()
    cnt = torch.tensor([3, 6], dtype=torch.int32, device=dev)
    want, _ = _run(c, name, [3, 6], "bilinear", bounded=False)
    step = DeviceFrameMasks(B, n, (H, W), dev, overlay=False)
    assert step.overlay is None
    fm = step(c["masks"]["bilinear"].to(dev), cnt, "bilinear", c["det"].to(dev), c["box"].to(dev))
    assert fm.bits is step.bits and fm.area is step.area and fm.overlay is None
    host = step.host()
    assert host.overlay is None and not host.bits.is_cuda
    assert torch.equal(host.bits.view(torch.int32), want.bits.view(torch.int32)) and torch.equal(host.area, want.area)
    with pytest.raises(ValueError):
        step(c["masks"]["bilinear"].to(dev), cnt, "bilinear", frames=torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev),
             records=torch.zeros((B, n, 8), device=dev))


def test_argument_errors_in_python():
    name = "18x22_to_45x70"
    mh, mw, H, W, n = SHAPES[name]
    c = _case(name)
    dev = _dev()
    masks, cnt = c["masks"]["bilinear"].to(dev), torch.tensor([3, 6], dtype=torch.int32, device=dev)
    det, box = c["det"].to(dev), c["box"].to(dev)
    frames = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev)
    rec = torch.zeros((B, n, 8), device=dev)
    for bad in (lambda: frame_masks(masks, cnt, (H, W), "bicubic"),
                lambda: frame_masks(masks, cnt, (H, 0)),
                lambda: frame_masks(masks.double(), cnt, (H, W)),
                lambda: frame_masks(masks, cnt.long(), (H, W)),
                lambda: frame_masks(masks[0], cnt, (H, W)),
                lambda: frame_masks(masks, cnt, (H, W), det=det),
                lambda: frame_masks(masks, cnt, (H, W), det=det[:, :3], box=box),
                lambda: frame_masks(masks, cnt, (H, W), frames=frames),
                lambda: frame_masks(masks, cnt, (H, W), frames=frames[:, :-1], records=rec),
                lambda: frame_masks(masks, cnt, (H, W), frames=frames, records=rec,
                                    palette=torch.zeros((0, 3), dtype=torch.uint8, device=dev)),
                lambda: frame_masks(masks.cpu(), cnt, (H, W)),
                lambda: frame_masks(masks, cnt, (H, W), out=FrameMasks(torch.zeros(1, device=dev), None, None)),
                lambda: frame_masks(masks.transpose(2, 3), cnt, (H, W))):
        with pytest.raises(ValueError):
            bad()
    # no detections at all: nothing is launched, the overlay is the frame
    fm = frame_masks(masks[:, :0], cnt, (H, W), frames=frames + 7, records=rec[:, :0])
    assert tuple(fm.bits.shape) == (B, 0, H, 3) and torch.equal(fm.overlay, frames + 7)


def test_c_abi_argument_errors():
    from tauv_vision_amd import _lib
    dev = _dev()
    L = _lib.lib()
    masks = torch.zeros((2, 3, 4, 5), device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    det = torch.zeros((2, 3), dtype=torch.int64, device=dev)
    box = torch.zeros((2, 5, 4), device=dev)
    frames = torch.zeros((2, 6, 40, 3), dtype=torch.uint8, device=dev)
    rec = torch.zeros((2, 3, 8), device=dev)
    pal = torch.zeros((10, 3), dtype=torch.uint8, device=dev)
    bits = torch.zeros((2, 3, 6, 2), dtype=torch.int32, device=dev)
    area = torch.zeros((2, 3), dtype=torch.int32, device=dev)
    over = torch.zeros((2, 6, 40, 3), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = _lib.stream_of(dev)

    def call(m=p(masks), mh=4, mw=5, counts=p(cnt), B_=2, n=3, H=6, W=40, mode=0, bound=1, dt=p(det), bx=p(box), A=5,
             fr=p(frames), rc=p(rec), pl=p(pal), nc=10, bt=p(bits), ar=p(area), ov=p(over)):
        return L.tv_yolact_frame_masks(m, mh, mw, counts, B_, n, H, W, mode, bound, dt, bx, A, fr, rc, pl, nc, bt, ar, ov, s)

    assert call() == _lib.TV_OK and call(mode=1) == _lib.TV_OK
    assert call(bound=0, dt=None, bx=None, A=0) == _lib.TV_OK
    assert call(fr=None, ov=None, rc=None, pl=None, nc=0) == _lib.TV_OK
    assert call(B_=0) == _lib.TV_OK and call(n=0, m=None, bt=None, ar=None) == _lib.TV_OK
    for bad in (dict(m=None), dict(counts=None), dict(bt=None), dict(ar=None), dict(mh=0), dict(mw=-1), dict(H=0),
                dict(W=0), dict(mode=2), dict(mode=-1), dict(dt=None), dict(bx=None), dict(A=0), dict(rc=None),
                dict(pl=None), dict(nc=0), dict(ov=None), dict(fr=None), dict(B_=-1), dict(n=-1)):
        assert call(**bad) == _lib.TV_EINVAL, bad
        assert L.tv_last_error().decode().startswith("frame_masks"), bad
    torch.cuda.synchronize()


# ---- YolactDetector(frame_masks=...) on test_gpu_yolact_detect's 72 x 88 model ----

def _detector_inputs():
    from recipe import seeded_u8_frames
    from test_gpu_resnet18 import IMG_H, IMG_W
    from test_gpu_yolact_detect import _graded_yolact, _threshold
    net = _graded_yolact("fp16")
    frames = seeded_u8_frames(B, IMG_H, IMG_W, seed=11).cuda()
    return net, frames, _threshold(net, frames), (IMG_H, IMG_W)


def _same(a, b, what):
    assert torch.equal(a.bits.view(torch.int32), b.bits.view(torch.int32)), what + ": bits"
    assert torch.equal(a.area, b.area), what + ": area"
    assert (a.overlay is None) == (b.overlay is None) and (a.overlay is None or torch.equal(a.overlay, b.overlay)), \
        what + ": overlay"


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_detector_equals_frame_masks_of_its_own_outputs(mode):
    from test_gpu_yolact_detect import IOU, TOP_K
    net, frames, thr, hw = _detector_inputs()
    dev = _dev()
    detector = tv.YolactDetector(net, B, hw, TOP_K, dev, frame_masks=mode)
    res = detector(frames, IOU, thr)
    counts = res.counts.cpu()
    assert any(0 < int(v) < TOP_K for v in counts), counts
    assert res.bits is detector.frame.bits and tuple(res.bits.shape) == (B, TOP_K, hw[0], (hw[1] + 31) // 32)
    for bounded in (True, False):
        want = frame_masks(res.masks, res.counts, hw, mode, det=detector.det if bounded else None,
                           box=detector.box if bounded else None, frames=frames, records=res.records)
        _same(FrameMasks(res.bits, res.area, res.overlay), want, f"detector vs frame_masks (bounded {bounded})")
    assert int(res.area.sum()) > 0 and not torch.equal(res.overlay, frames)
    for b in range(B):
        assert not res.area[b, int(counts[b]):].any()
    host = detector.host_frame_masks()
    assert not host.bits.is_cuda
    _same(host, FrameMasks(res.bits.cpu(), res.area.cpu(), res.overlay.cpu()), "host_frame_masks")
    # Yolact.detect passes the option on, with a detector of its own per option
    got = net.detect(frames, TOP_K, IOU, thr, frame_masks=mode)
    _same(FrameMasks(got.bits, got.area, got.overlay), FrameMasks(res.bits, res.area, res.overlay), "Yolact.detect")
    plain = net.detect(frames, TOP_K, IOU, thr)
    assert plain.bits is None and plain.area is None and plain.overlay is None
    assert torch.equal(plain.records, got.records)
    # the fp32 entry has no frames to draw on
    img = tv.preprocess(frames, *hw)
    res32 = detector(img, IOU, thr)
    assert res32.overlay is None and res32.bits is detector.frame.bits
    assert detector.host_frame_masks().overlay is None
    with pytest.raises(ValueError):
        tv.YolactDetector(net, B, hw, TOP_K, dev, frame_masks="bicubic")
    with pytest.raises(ValueError):
        net.detect(frames, TOP_K, IOU, thr, frame_masks="cubic")


def test_detector_graph_replay_on_a_frame_with_fewer_detections():
    """The stale-row case: the graph is captured and replayed on frames with more detections, then
    replayed on frames with fewer; every output must equal an eager call on those frames."""
    from recipe import seeded_u8_frames
    from test_gpu_yolact_detect import IOU, TOP_K
    net, frames, thr, hw = _detector_inputs()
    dev = _dev()
    probe = tv.YolactDetector(net, B, hw, TOP_K, dev, frame_masks="bilinear")
    candidates = [frames] + [seeded_u8_frames(B, hw[0], hw[1], seed=s).cuda() for s in (12, 13, 14, 15)] + \
        [torch.full_like(frames, 128)]
    eager = []
    for f in candidates:
        r = probe(f, IOU, thr)
        eager.append(dict(counts=r.counts.cpu().clone(), bits=r.bits.clone(), area=r.area.clone(),
                          overlay=r.overlay.clone(), records=r.records.clone()))
    totals = [int(e["counts"].sum()) for e in eager]
    print("detections per candidate frame pair:", [e["counts"].tolist() for e in eager])
    first, second = totals.index(max(totals)), totals.index(min(totals))
    assert totals[second] < totals[first], "the candidate frames all give the same number of detections"
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        detector = tv.YolactDetector(net, B, hw, TOP_K, dev, frame_masks="bilinear")
        buf = candidates[first].clone()
        detector(buf, IOU, thr)  # the eager step on the capture stream
        s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = detector(buf, IOU, thr)
    for i in (first, second):
        buf.copy_(candidates[i])
        graph.replay()
        torch.cuda.synchronize()
        e = eager[i]
        assert torch.equal(res.counts.cpu(), e["counts"])
        assert torch.equal(res.records, e["records"])
        _same(FrameMasks(res.bits, res.area, res.overlay), FrameMasks(e["bits"], e["area"], e["overlay"]),
              f"replay on candidate {i}")


def test_detector_without_frame_masks_is_the_parents_sequence():
    from test_gpu_yolact_detect import CAMERA, IOU, TOP_K, _depth, _equal_detections, _one_by_one
    net, frames, thr, hw = _detector_inputs()
    depth = _depth(B).cuda()
    detector = tv.YolactDetector(net, B, hw, TOP_K, _dev())
    assert detector.frame is None and detector.frame_mode is None
    res = detector(frames, IOU, thr, depth, CAMERA)
    assert res.bits is None and res.area is None and res.overlay is None
    _equal_detections(res, detector.det, _one_by_one(net, frames, thr, depth), "frame_masks=None vs the steps")
    with pytest.raises(ValueError):
        detector.host_frame_masks()
