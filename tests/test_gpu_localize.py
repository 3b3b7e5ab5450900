"""GPU depth localisation of detections (csrc/localize.hip) against tests/localize_ref.py, the host
restatement of the two reference nodes' loops (centernet_node.py:139-178, yolact_node.py:135-193).

Comparison rules (localize_ref.compare_row): valid and n_pixels exact; e_x, e_y the float64
reference rounded to fp32; depth_sum, z, x, y at rtol 1.2e-7, atol 0 — the kernel's integer sum is
exact and the reference's pairwise float64 sum within ~1e-14, so their fp32 roundings differ by at
most one fp32 ulp (2^-23). The threshold tests can differ only within ~1e-13 of equality: every
input set is first checked on the CPU to keep depth_sum and z at least 1e-6 from its threshold."""
import types

import numpy as np
import pytest
import torch

import localize_ref as ref
import tauv_vision_amd as tv
from tauv_vision_amd.decode import DeviceDecoder
from tauv_vision_amd.yolact import assemble_masks_indexed

pytestmark = pytest.mark.gpu

M = np.array([[411.3, 0.0, 31.7], [0.0, 409.9, 18.2], [0.0, 0.0, 0.0]])
CAM = (411.3, 409.9, 31.7, 18.2)
NAN, INF = float("nan"), float("inf")


def _dev():
    return torch.device("cuda", 0)


def _box_depth(dh, dw, seed):
    """1.1 .. 3 m everywhere (so three pixels sum to < 10 m and z >= 1.1), ~10 % zeros off column 0,
    0.5 .. 0.7 m in rows 0-9 x columns 0-15 (z < 1) and zeros in rows 24.. x columns 40-55."""
    rng = np.random.default_rng(seed)
    d = rng.integers(1100, 3001, size=(dh, dw)).astype(np.uint16)
    zero = rng.random((dh, dw)) < 0.1
    zero[:, 0] = False
    d[zero] = 0
    d[17, 11] = 2000  # the one-pixel case's pixel holds depth
    d[0:10, 0:16] = rng.integers(500, 701, size=(10, 16))
    d[24:, 40:56] = 0
    return d


def _box_cases(dh, dw):
    """(name, (y, x, h, w)) with the box given in depth pixels: centre (cx, cy), size (w, h)."""
    def px(cx, cy, w, h):
        return (cy / dh, cx / dw, h / dh, w / dw)

    return [
        ("interior", px(30.3, 17.6, 20, 10)),
        ("clipped left", px(2, 18, 20, 10)),
        ("clipped right", px(dw - 2, 18, 20, 10)),
        ("clipped top", px(30, 1, 16, 12)),
        ("clipped bottom", px(30, dh - 1, 16, 12)),
        ("wholly outside", px(-30, 10, 10, 10)),
        ("outside, corner in (-1, 0): column 0", px(-1.5, 18, 2, 20)),
        ("outside, corner in (-1, 0): row 0", px(30, -1.5, 20, 2)),
        ("negative w", px(30, 17, -20, 10)),
        ("negative h", px(30, 17, 20, -10)),
        ("w = h = 0: one pixel", px(11.5, 17.5, 0, 0)),
        ("all-zero depth", px(47.5, 29.5, 10, 6)),
        ("sum >= 10, z < 1", px(7.5, 4.5, 16, 8)),
        ("sum < 10", px(30.5, 17.5, 2.6, 0)),
        ("contraction: x = 3/64, w = 5/64", (18 / dh, 3 / 64, 10 / dh, 5 / 64)),
        ("NaN w", (0.5, 0.5, 0.2, NAN)),
        ("inf h", (0.5, 0.5, INF, 0.2)),
        ("NaN x", (0.5, NAN, 0.2, 0.2)),
        ("-inf y", (-INF, 0.5, 0.2, 0.2)),
        ("odd start column", px(20.5, 18, 12.5, 8)),
        ("huge w, h: the whole frame", (0.5, 0.5, 1e30, 1e30)),
        ("far off to the right", px(1e12, 18, 20, 10)),
        ("wide: one row, many vectors", px(32, 3.5, 200, 0)),
        ("tall: one column", px(33.5, 18, 0, 200)),
        ("top-left corner", px(1, 1, 6, 6)),
        ("bottom-right corner", px(dw - 1, dh - 1, 7, 7)),
    ]


def _chunks(cases):
    """B = 2, K = 8, counts [8, 5]: 13 cases per launch; rows 5-7 of image 1 hold a plausible box that
    is past its count."""
    past = ("past counts", (0.5, 0.5, 0.5, 0.5))
    for i in range(0, len(cases), 13):
        c = cases[i:i + 13]
        c = c + [cases[0]] * (13 - len(c))
        yield [c[:8], c[8:13] + [past] * 3]


def _check_boxes(out, images, depth_np, counts, thresholds, what):
    out = out.cpu().numpy()
    for b, img in enumerate(images):
        dets = [tuple(float(np.float32(v)) for v in yxhw) for _, yxhw in img[:counts[b]]]
        want = ref.centernet_localize(dets, depth_np[b if depth_np.shape[0] > 1 else 0], M, 0.4, *thresholds)
        ref.assert_clear_of_thresholds(want, *thresholds)
        for k, r in enumerate(want):
            ref.compare_row(out[b, k], r, f"{what} / {img[k][0]}")
        assert not out[b, counts[b]:].any(), f"{what}: rows past counts[{b}] are not zero"
    return out


@pytest.mark.parametrize("thresholds", [(10.0, 1.0), (0.0, 0.0)])
@pytest.mark.parametrize("dh,dw", [(36, 64), (37, 63)])
def test_box_mode(dh, dw, thresholds):
    dev = _dev()
    depth_np = np.stack([_box_depth(dh, dw, 1), _box_depth(dh, dw, 2)])
    depth = torch.from_numpy(depth_np).to(dev)
    counts_l = [8, 5]
    counts = torch.tensor(counts_l, dtype=torch.int32, device=dev)
    loc = tv.DeviceLocalizer(2, 8, dev)
    n_valid, seen = 0, {}
    for images in _chunks(_box_cases(dh, dw)):
        rec = np.full((2, 8, 10), np.nan, dtype=np.float32)  # only columns 2-5 are read
        for b in range(2):
            for k in range(8):
                rec[b, k, 2:6] = np.array(images[b][k][1], dtype=np.float32)
        loc.out.fill_(float("nan"))
        out = loc.boxes(torch.from_numpy(rec).to(dev), counts, depth, *CAM, 0.4, *thresholds)
        assert out is loc.out
        got = _check_boxes(out, images, depth_np, counts_l, thresholds, f"{dh}x{dw}")
        n_valid += int(got[..., 3].sum())
        for b in range(2):
            for k in range(counts_l[b]):
                seen[images[b][k][0]] = got[b, k]
    # the cases select what they are named for
    assert seen["wholly outside"][4] == 0
    assert seen["outside, corner in (-1, 0): column 0"][4] > 0
    assert seen["outside, corner in (-1, 0): row 0"][4] > 0
    assert 0 < seen["w = h = 0: one pixel"][4] <= 1
    assert seen["all-zero depth"][4] == 0
    assert seen["huge w, h: the whole frame"][4] == np.count_nonzero(depth_np[0]) or \
        seen["huge w, h: the whole frame"][4] == np.count_nonzero(depth_np[1])
    if thresholds == (10.0, 1.0):
        assert seen["sum >= 10, z < 1"][3] == 0 and seen["sum >= 10, z < 1"][5] >= 10
        assert seen["sum < 10"][3] == 0 and 0 < seen["sum < 10"][5] < 10
    else:
        assert seen["sum >= 10, z < 1"][3] == 1 and seen["sum < 10"][3] == 1
    assert n_valid >= 10


def test_contraction_example_selects_column_1():
    """x = 3/64, w = 5/64 at dw = 64: the left corner is 3 - 2.0 = 1.0 (column 1); an FMA gives
    0.9999999999999999 (column 0). Only column 0 holds depth, so a contracted corner shows."""
    dev = _dev()
    depth_np = np.zeros((1, 36, 64), dtype=np.uint16)
    depth_np[0, :, 0] = 2000
    rec = np.zeros((1, 1, 10), dtype=np.float32)
    rec[0, 0, 2:6] = (0.5, 3 / 64, 0.5, 5 / 64)
    loc = tv.DeviceLocalizer(1, 1, dev)
    out = loc.boxes(torch.from_numpy(rec).to(dev), torch.ones(1, dtype=torch.int32, device=dev),
                    torch.from_numpy(depth_np).to(dev), *CAM, 0.4, 0.0, 0.0).cpu().numpy()
    want, = ref.centernet_localize([(0.5, 3 / 64, 0.5, 5 / 64)], depth_np[0], M, 0.4, 0, 0)
    assert want["n_pixels"] == 0
    ref.compare_row(out[0, 0], want, "contraction")


def test_overflow_of_32_bit_sums():
    dev = _dev()
    depth_np = np.full((1, 264, 256), 65535, dtype=np.uint16)
    rec = np.zeros((1, 1, 10), dtype=np.float32)
    rec[0, 0, 2:6] = (0.5, 0.5, 2.0, 2.0)
    loc = tv.DeviceLocalizer(1, 1, dev)
    out = loc.boxes(torch.from_numpy(rec).to(dev), torch.ones(1, dtype=torch.int32, device=dev),
                    torch.from_numpy(depth_np).to(dev), *CAM).cpu().numpy()
    assert out[0, 0, 4] == 67584 and out[0, 0, 3] == 1
    assert abs(float(out[0, 0, 5]) - 4429117.44) <= 1.2e-7 * 4429117.44
    assert abs(float(out[0, 0, 2]) - 65.535) <= 1.2e-7 * 65.535
    want, = ref.centernet_localize([(0.5, 0.5, 2.0, 2.0)], depth_np[0], M)
    ref.compare_row(out[0, 0], want, "overflow")


def test_depth_broadcast():
    dev = _dev()
    dh, dw = 37, 63
    d1 = _box_depth(dh, dw, 3)[None]
    images = next(_chunks(_box_cases(dh, dw)))
    rec = np.zeros((2, 8, 10), dtype=np.float32)
    for b in range(2):
        for k in range(8):
            rec[b, k, 2:6] = np.array(images[b][k][1], dtype=np.float32)
    rec_d = torch.from_numpy(rec).to(dev)
    counts = torch.tensor([8, 5], dtype=torch.int32, device=dev)
    a = tv.DeviceLocalizer(2, 8, dev).boxes(rec_d, counts, torch.from_numpy(d1).to(dev), *CAM)
    b = tv.DeviceLocalizer(2, 8, dev).boxes(rec_d, counts, torch.from_numpy(np.repeat(d1, 2, axis=0)).to(dev), *CAM)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _check_boxes(a, images, d1, [8, 5], (10.0, 1.0), "broadcast")
    assert a[..., 3].sum() > 0


def _mask_inputs(dh, dw, mh, mw, seed):
    g = torch.Generator().manual_seed(seed)
    B, n, A = 2, 3, 6
    masks = torch.rand((B, n, mh, mw), generator=g)
    masks[torch.rand((B, n, mh, mw), generator=g) < 0.2] = 0.5  # exactly 0.5: not selected
    masks[0, 2] = torch.rand((mh, mw), generator=g) * 0.5       # nothing above 0.5: an invalid row
    masks[0, 2, 0, 0] = 0.5
    det = torch.randint(0, A, (B, n), generator=g)
    box = torch.rand((B, A, 4), generator=g)
    rng = np.random.default_rng(seed)
    depth = rng.integers(300, 65536, size=(B, dh, dw)).astype(np.uint16)
    depth[rng.random((B, dh, dw)) < 0.3] = 0
    return masks, det, box, depth


def _check_masks(out, masks, det, box, depth_np, counts, what):
    out = out.cpu().numpy()
    for b in range(masks.shape[0]):
        c = counts[b]
        want = ref.yolact_localize(masks[b, :c], det[b, :c].tolist(), box[b], depth_np[b], *CAM)
        ref.assert_clear_of_thresholds(want, 0.0, 0.0)
        for k, r in enumerate(want):
            ref.compare_row(out[b, k], r, f"{what} / image {b} detection {k}")
        assert not out[b, c:].any(), f"{what}: rows past counts[{b}] are not zero"
    return out


@pytest.mark.parametrize("dh,dw,mh,mw", [(50, 550, 9, 45), (550, 50, 45, 9), (50, 550, 7, 5), (550, 50, 7, 5)])
def test_mask_mode(dh, dw, mh, mw):
    dev = _dev()
    masks, det, box, depth_np = _mask_inputs(dh, dw, mh, mw, 7)
    counts_l = [3, 2]
    loc = tv.DeviceLocalizer(2, 3, dev)
    loc.out.fill_(float("nan"))
    out = loc.masks(masks.to(dev), torch.tensor(counts_l, dtype=torch.int32, device=dev), det.to(dev), box.to(dev),
                    torch.from_numpy(depth_np).to(dev), *CAM)
    got = _check_masks(out, masks, det, box, depth_np, counts_l, f"{mh}x{mw} -> {dh}x{dw}")
    assert got[0, 2, 3] == 0 and got[0, 2, 4] == 0, "a mask that is nowhere above 0.5 selects nothing"
    assert got[0, 0, 3] == 1 and got[0, 1, 3] == 1 and got[1, 0, 3] == 1 and got[1, 1, 3] == 1
    # the host-record form of the same call
    host = tv.localize_masks(masks, det, box, depth_np, *CAM, counts=torch.tensor(counts_l, dtype=torch.int32))
    assert np.array_equal(host.view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("dh,dw,mh,mw", [(50, 550, 9, 45), (550, 50, 45, 9), (50, 550, 7, 5)])
def test_mask_mode_bound_by_box_is_bit_equal(dh, dw, mh, mw):
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    B, n, A, P = 2, 3, 6, 8
    proto = torch.randn((B, P, mh, mw), generator=g).to(dev)
    coeff = torch.randn((B, A, P), generator=g).to(dev)
    box = torch.cat([0.15 + 0.7 * torch.rand((B, A, 2), generator=g), 0.1 + 0.5 * torch.rand((B, A, 2), generator=g)],
                    dim=-1)
    box[0, 0] = torch.tensor([0.02, 0.97, 0.3, 0.3])  # crop clipped at two edges
    det = torch.randint(0, A, (B, n), generator=g)
    det[0, 0] = 0
    counts_l = [3, 2]
    counts = torch.tensor(counts_l, dtype=torch.int32, device=dev)
    masks = assemble_masks_indexed(proto, coeff, box.to(dev), det.to(dev), counts,
                                   out=torch.zeros((B, n, mh, mw), device=dev))
    _, _, _, depth_np = _mask_inputs(dh, dw, mh, mw, 13)
    depth = torch.from_numpy(depth_np).to(dev)
    full = tv.DeviceLocalizer(B, n, dev).masks(masks, counts, det.to(dev), box.to(dev), depth, *CAM)
    crop = tv.DeviceLocalizer(B, n, dev).masks(masks, counts, det.to(dev), box.to(dev), depth, *CAM,
                                               bound_by_box=True)
    assert torch.equal(full.view(torch.int32), crop.view(torch.int32))
    got = _check_masks(full, masks.cpu(), det, box, depth_np, counts_l, "assembled masks")
    assert got[..., 4].sum() > 0


def test_chain_decoder_records_and_node_call_agree():
    dev = _dev()
    g = torch.Generator().manual_seed(3)
    B, C, H, W, K, ratio = 2, 4, 24, 32, 8, 4
    heat = -6.0 + 0.1 * torch.randn((B, C, H, W), generator=g)
    peaks = [[(0, 3, 4), (1, 12, 16), (2, 20, 28), (3, 7, 22), (0, 18, 9)], [(1, 5, 5), (2, 12, 20), (3, 19, 12)]]
    for b, img in enumerate(peaks):  # 5 and 3 detections above the threshold, the other slots below it
        for i, (c, y, x) in enumerate(img):
            heat[b, c, y, x] = 2.0 + 0.3 * i
    # Prediction layout: heatmap [B, C, H, W], size / offset [B, H, W, 2]
    pred = types.SimpleNamespace(heatmap=heat.to(dev),
                                 size=(0.1 + torch.rand((B, H, W, 2), generator=g) * 0.3).to(dev),
                                 offset=(torch.rand((B, H, W, 2), generator=g) * ratio).to(dev), depth=None)
    mc = tv.ModelConfig([2] * 5, [16] * 6, H * ratio, W * ratio, 2, 1.0)
    assert mc.downsample_ratio == ratio
    thr = 0.5
    depth_np = np.random.default_rng(5).integers(1100, 3001, size=(B, 45, 80)).astype(np.uint16)
    dec = DeviceDecoder(B, C, H, W, K, dev)
    records, counts = dec(pred.heatmap, pred.size, pred.offset, None, 0, ratio, mc.in_h, mc.in_w, thr)
    loc = tv.DeviceLocalizer(B, K, dev)
    out = loc.boxes(records, counts, torch.from_numpy(depth_np).to(dev), M[0, 0], M[1, 1], M[0, 2], M[1, 2])
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    dets = tv.decode(pred, mc, K, thr)
    pts = tv.localize_detections(dets, depth_np, M)
    assert [len(p) for p in pts] == [len(d) for d in dets] == counts.tolist()
    n_valid = 0
    for b in range(B):
        for k, p in enumerate(pts[b]):
            if p is None:
                assert out[b, k, 3] == 0
            else:
                assert out[b, k, 3] == 1 and p == tuple(float(v) for v in out[b, k, :3])
                n_valid += 1
        # one image's list on its own
        assert tv.localize_detections([dets[b]], depth_np[b], M) == [pts[b]]
    assert counts.tolist() == [5, 3] and n_valid > 0


def _bits(t):
    return t.view(torch.int32)


def test_graph_replay_rewrites_every_row():
    dev = _dev()
    dh, dw, mh, mw = 37, 63, 7, 5
    chunks = list(_chunks(_box_cases(dh, dw)))

    def box_inputs(i, counts_l):
        rec = np.zeros((2, 8, 10), dtype=np.float32)
        for b in range(2):
            for k in range(8):
                rec[b, k, 2:6] = np.array(chunks[i][b][k][1], dtype=np.float32)
        return (torch.from_numpy(rec).to(dev), torch.tensor(counts_l, dtype=torch.int32, device=dev),
                torch.from_numpy(np.stack([_box_depth(dh, dw, 20 + i), _box_depth(dh, dw, 30 + i)])).to(dev))

    def mask_inputs(seed, counts_l):
        masks, det, box, depth_np = _mask_inputs(dh, dw, mh, mw, seed)
        return (masks.to(dev), torch.tensor(counts_l, dtype=torch.int32, device=dev), det.to(dev), box.to(dev),
                torch.from_numpy(depth_np).to(dev))

    first_b, first_m = box_inputs(0, [8, 5]), mask_inputs(40, [3, 2])
    second_b, second_m = box_inputs(1, [2, 8]), mask_inputs(41, [1, 3])
    static_b, static_m = [t.clone() for t in first_b], [t.clone() for t in first_m]
    loc_b, loc_m = tv.DeviceLocalizer(2, 8, dev), tv.DeviceLocalizer(2, 3, dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        loc_b.boxes(*static_b, *CAM)
        loc_m.masks(*static_m, *CAM)
        s.synchronize()
    torch.cuda.current_stream(dev).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        loc_b.boxes(*static_b, *CAM)
        loc_m.masks(*static_m, *CAM)
    for inputs_b, inputs_m in ((second_b, second_m), (first_b, first_m)):
        for dst, src in zip(static_b + static_m, list(inputs_b) + list(inputs_m)):
            dst.copy_(src)
        loc_b.out.fill_(float("nan"))
        loc_m.out.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        want_b = tv.DeviceLocalizer(2, 8, dev).boxes(*inputs_b, *CAM)
        want_m = tv.DeviceLocalizer(2, 3, dev).masks(*inputs_m, *CAM)
        torch.cuda.synchronize()
        assert torch.equal(_bits(loc_b.out), _bits(want_b)), "replayed box rows differ from the eager call"
        assert torch.equal(_bits(loc_m.out), _bits(want_m)), "replayed mask rows differ from the eager call"
    assert want_b[..., 3].sum() > 0 and want_m[..., 3].sum() > 0


def test_c_abi_argument_errors():
    import ctypes
    from tauv_vision_amd import _lib
    dev = _dev()
    L = _lib.lib()
    rec = torch.zeros((2, 3, 10), device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    depth = torch.zeros((2, 4, 6), dtype=torch.uint16, device=dev)
    out = torch.zeros((2, 3, 8), device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = _lib.stream_of(dev)

    def boxes(records=p(rec), counts=p(cnt), B=2, K=3, d=p(depth), db=2, dh=4, dw=6, fx=1.0, fy=1.0, o=p(out)):
        return L.tv_localize_boxes(records, 10, counts, B, K, d, db, dh, dw, 0.4, fx, fy, 0.0, 0.0, 10.0, 1.0, o, s)

    assert boxes() == _lib.TV_OK
    assert boxes(B=0) == _lib.TV_OK and boxes(K=0, records=None) == _lib.TV_OK
    for bad in (dict(records=None), dict(counts=None), dict(d=None), dict(o=None), dict(dh=0), dict(dw=-1),
                dict(db=3), dict(fx=0.0), dict(fy=0.0), dict(B=-1)):
        assert boxes(**bad) == _lib.TV_EINVAL, bad
        assert L.tv_last_error().decode().startswith("localize_boxes"), bad
    det = torch.zeros((2, 3), dtype=torch.int64, device=dev)
    box = torch.zeros((2, 5, 4), device=dev)
    masks = torch.zeros((2, 3, 2, 3), device=dev)

    def mk(m=p(masks), mh=2, mw=3, counts=p(cnt), dt=p(det), bx=p(box), A=5, B=2, n=3, d=p(depth), db=1, fx=1.0,
           o=p(out)):
        return L.tv_localize_masks(m, mh, mw, counts, dt, bx, A, B, n, d, db, 4, 6, 0, fx, 1.0, 0.0, 0.0, 0.0, 0.0, o, s)

    assert mk() == _lib.TV_OK and mk(n=0) == _lib.TV_OK
    for bad in (dict(m=None), dict(dt=None), dict(bx=None), dict(counts=None), dict(d=None), dict(o=None), dict(mh=0),
                dict(mw=0), dict(A=0), dict(db=3), dict(fx=0.0)):
        assert mk(**bad) == _lib.TV_EINVAL, bad
        assert L.tv_last_error().decode().startswith("localize_masks"), bad
    torch.cuda.synchronize()
