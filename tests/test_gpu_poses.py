"""tv_solve_poses (csrc/pose.hip) and what is built on it - DevicePoseSolver, DeviceKeypointDecoder(poses=True),
decode_keypoint_poses, decode_keypoints(pose="device"), CenternetDetector(poses=True), detect_keypoints -
against the float64 restatement of the contract (pnp_ref.py) on the same fp32 inputs.

Bar: the rotation's geodesic angle, |dt| / |t| and the relative rms difference are at most max(4 e_ref,
2^-20), e_ref the distance between the restatement's linearly started and truth-started runs after rounding
to the fp32 output; valid, n and the NaN pattern exactly. Frames are 360 x 640 with cx = 320, cy = 180, so
a y / x or in_h / in_w swap cannot pass."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import pnp_ref as P

pytestmark = pytest.mark.gpu

MODELS, M_PROJ, (FRAME_H, FRAME_W) = P.load_models()
CAM = (M_PROJ[0, 0], M_PROJ[1, 1], M_PROJ[0, 2], M_PROJ[1, 2])
PLANAR = (2,)


def _table():
    return P.model_table([MODELS["eight"], MODELS["seven"], P.octagon(), np.zeros((1, 3))])


def _raw(arrays, table, cam=CAM, min_points=6, in_h=FRAME_H, in_w=FRAME_W, **override):
    """tv_solve_poses itself on host arrays: (return code, poses numpy). The output starts at a sentinel."""
    from tauv_vision_amd import _lib
    dev = torch.device("cuda", 0)
    rec, cnt, kp, kcnt, slot = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)
    tab = torch.from_numpy(np.ascontiguousarray(table)).to(dev)
    B, K = rec.shape[:2]
    out = torch.full((B, K, 16), 7.0, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    a = dict(rec=vp(rec), cnt=vp(cnt), kp=vp(kp), kcnt=vp(kcnt), slot=vp(slot), tab=vp(tab), n_labels=table.shape[0],
             S=table.shape[1], B=B, K=K, K_kp=kp.shape[1], in_h=in_h, in_w=in_w, fx=cam[0], fy=cam[1], cx=cam[2],
             cy=cam[3], min_points=min_points, out=vp(out))
    a.update(override)
    rc = _lib.lib().tv_solve_poses(a["rec"], a["cnt"], a["kp"], a["kcnt"], a["slot"], a["tab"], a["n_labels"], a["S"],
                                   a["B"], a["K"], a["K_kp"], a["in_h"], a["in_w"], a["fx"], a["fy"], a["cx"], a["cy"],
                                   a["min_points"], a["out"], _lib.stream_of(dev))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _check(arrays, table, truths, got, what, cam=CAM, in_h=FRAME_H, in_w=FRAME_W):
    ref, bars = P.reference_and_bars(arrays, table, in_h, in_w, cam, truths)
    worst = P.assert_poses(got, ref, bars, what)
    print(f"{what}: {int(ref[..., 12].sum())} valid rows, worst angle / |dt|/|t| / rms {worst}, largest bar "
          f"{bars.max(axis=(0, 1))}, at most {int(np.nanmax(got[..., 15]))} iterations")
    return ref


@pytest.mark.parametrize("variant", ["five_points", "bad_label"])
def test_hand_made_records(variant):
    table, rng = _table(), np.random.default_rng(21)
    K, K_kp = 4, 40
    arrays = list(P.random_batch(rng, table, PLANAR, 2, K, K_kp, [4, 4], FRAME_H, FRAME_W, CAM))
    truths = arrays.pop()
    rec, cnt, kp, kcnt, slot = arrays
    # image 0: the 8-point model exact with two slots unmatched, the 7-point model with noise and one slot
    # past the keypoint count, the planar model with noise, and the variant's row
    poses = {0: P.random_pose(rng), 1: P.random_pose(rng), 2: P.tilted_pose(rng), 3: P.random_pose(rng)}
    labels = [0, 1, 2, 1]
    dets = []
    for d, l in enumerate(labels):
        obj = table[l][~np.isnan(table[l, :, 0])].astype(np.float64)
        uv, _ = P.project(*poses[d], obj, CAM)
        if d in (1, 2):
            uv = uv + rng.normal(scale=0.5, size=uv.shape)
        gone = {0: (2, 5), 3: (0, 6) if variant == "five_points" else ()}.get(d, ())
        dets.append((l, {s: tuple(uv[s]) for s in range(len(obj)) if s not in gone}))
    r0 = P.make_records([dets], K, K_kp, 8, FRAME_H, FRAME_W)
    for dst, src in zip((rec, kp, slot), (r0[0], r0[2], r0[4])):
        dst[0] = src[0]
    kcnt[0] = r0[3][0]
    slot[0, 1, 4] = kcnt[0] + 3          # a rank past the keypoint count: not a point
    cnt[:] = (4, 0)                      # the second image's rows are filled but not counted
    if variant == "bad_label":
        rec[0, 3, 0] = 7                 # outside [0, n_labels)
        rec[0, 2, 0] = 3                 # and the planar row becomes the one-keypoint label
    truths = {(0, d): poses[d] for d in range(4)}
    rc, got = _raw((rec, cnt, kp, kcnt, slot), table)
    assert rc == 0
    ref = _check((rec, cnt, kp, kcnt, slot), table, truths, got, f"hand-made ({variant})")
    assert ref[0, 0, 12:14].tolist() == [1, 6] and ref[0, 1, 12:14].tolist() == [1, 6]
    if variant == "five_points":
        assert ref[0, 2, 12:14].tolist() == [1, 8] and ref[0, 3, 12:14].tolist() == [0, 5]
    else:
        assert ref[0, 2, 12:14].tolist() == [0, 1] and ref[0, 3, 12:14].tolist() == [0, 0]
    assert (got[1, :, 12:14] == 0).all() and np.isnan(got[1, :, 0:12]).all() and (got[1, :, 15] == 0).all()
    # the exact 6-point row recovers its pose: nothing was swapped on the way in
    assert P.geodesic(got[0, 0, 0:9].reshape(3, 3), poses[0][0]) <= 1e-5


def test_more_detections_than_one_workgroup_and_ragged_counts():
    table, rng = _table(), np.random.default_rng(22)
    B, K, K_kp, counts = 3, 70, 600, [70, 0, 37]
    *arrays, truths = P.random_batch(rng, table, PLANAR, B, K, K_kp, counts, FRAME_H, FRAME_W, CAM,
                                     drop={(0, 5): (1,), (2, 8): (0, 3), (2, 9): (0, 3, 4)})
    rc, got = _raw(arrays, table)
    assert rc == 0
    ref = _check(arrays, table, truths, got, "B = 3, K = 70")
    assert ref[0, 5, 12] == 1 and ref[2, 9, 12] == 0 and ref[2, 9, 13] in (4, 5) and int(ref[..., 12].sum()) >= 100
    assert (got[1, :, 13] == 0).all() and (got[2, 37:, 13] == 0).all()


def test_degenerate_rows_do_not_disturb_their_neighbours():
    table, rng = _table(), np.random.default_rng(23)
    table = np.concatenate([table, np.tile(np.float32([[0.1, 0.2, 0.3]]), (1, 8, 1))])  # label 4: all points equal
    K, K_kp = 6, 60
    *arrays, truths = P.random_batch(rng, table[:4], PLANAR, 1, K, K_kp, [6], FRAME_H, FRAME_W, CAM)
    rec, cnt, kp, kcnt, slot = arrays
    kp[0, slot[0, 1, 3], 2] = np.nan                    # a NaN keypoint
    kp[0, slot[0, 2, :8][slot[0, 2, :8] >= 0], 2:4] = (0.4, 0.6)  # every keypoint of the object at one pixel
    rec[0, 3, 0] = 4                                    # a model whose points are all equal
    for d in (1, 2, 3):
        truths.pop((0, d))
    rc, got = _raw(arrays, table)
    assert rc == 0
    ref = _check(arrays, table, truths, got, "degenerate rows")
    assert ref[0, :, 12].tolist() == [1, 0, 0, 0, 1, 1]
    clean = list(P.random_batch(np.random.default_rng(23), table[:4], PLANAR, 1, K, K_kp, [6], FRAME_H, FRAME_W, CAM))[:5]
    _, alone = _raw(clean, table)
    for d in (0, 4, 5):
        assert np.array_equal(got[0, d], alone[0, d]), "a good row changed next to degenerate ones"


def _planted(B, seed, in_h=FRAME_H, in_w=FRAME_W, cam=CAM, tz=(0.5, 0.7)):
    import tauv_vision_amd as tv
    from tauv_vision_amd.centernet import Prediction
    oc = P.four_label_config(tv)
    mc = tv.ModelConfig([1], [1], in_h, in_w, 2, 1.0)
    heads, truths = P.planted_heads(B, in_h // 4, in_w // 4, 4, oc, cam, seed, tz=tz)
    fields = {f: None for f in Prediction.__dataclass_fields__}
    fields.update({k: v.cuda() for k, v in heads.items()})
    return tv, oc, mc, Prediction(**fields), truths


def test_decoder_with_poses_keeps_its_prefix_and_equals_the_solver():
    tv, oc, mc, pred, truths = _planted(2, 31)
    dev = torch.device("cuda", 0)
    B, C, H, W = pred.heatmap.shape
    K, K_kp = 5, 40
    plain = tv.DeviceKeypointDecoder(B, C, oc.n_keypoints, H, W, K, K_kp, oc, dev)
    dec = tv.DeviceKeypointDecoder(B, C, oc.n_keypoints, H, W, K, K_kp, oc, dev, poses=True)
    assert plain.poses is None and dec.packed.numel() == plain.packed.numel() + B * K * 16 * 4
    with pytest.raises(ValueError, match="poses=True"):
        plain.solve(mc, CAM)
    plain(pred, mc, 0.5, 0.5)
    res = dec(pred, mc, 0.5, 0.5)
    poses = dec.solve(mc, CAM)
    torch.cuda.synchronize()
    n = plain.packed.numel()
    assert torch.equal(dec.packed[:n], plain.packed), "the prefix of packed changed with poses=True"
    assert poses.data_ptr() == dec.packed.data_ptr() + n and res.counts.tolist() == [1, 1]
    assert res.n_matched[:, 0].tolist() == [8, 8]
    solver = tv.DevicePoseSolver(B, K, K_kp, oc, dev)
    alone = solver(res.records, res.counts, res.keypoint_records, res.keypoint_counts, res.slot_kp, mc, CAM)
    assert torch.equal(alone.view(torch.int32), poses.view(torch.int32))
    host = dec.host()
    hp = dec.host_poses()
    assert torch.equal(hp.view(torch.int32), poses.cpu().view(torch.int32)) and isinstance(host, tv.KeypointRecords)
    arrays = tuple(getattr(host, f).numpy() for f in ("records", "counts", "keypoint_records", "keypoint_counts", "slot_kp"))
    ref = _check(arrays, tv.pose_model_points(oc), truths, hp.numpy(), "planted 90 x 160")
    assert ref[:, 0, 12].tolist() == [1, 1]
    # the same through the one-call API and the detection objects
    rec, p2 = tv.decode_keypoint_poses(pred, mc, oc, M_PROJ, K, K_kp, 0.5, 0.5)
    assert np.array_equal(p2.view(np.int32), hp.numpy().view(np.int32)) and np.array_equal(rec.slot_kp, arrays[4])
    dets = tv.decode_keypoints(pred, mc, oc, M_PROJ, K, K_kp, 0.5, 0.5, 0.0, pose="device")
    for b in range(B):
        R, t = dets[b][0].cam_t_object
        assert np.array_equal(R, p2[b, 0, 0:9].astype(np.float64).reshape(3, 3)) and t.shape == (3, 1)
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="solvePnP needs OpenCV"):
            tv.decode_keypoints(pred, mc, oc, M_PROJ, K, K_kp, 0.5, 0.5, 0.0)
    # refusals of the solver, before any launch
    before = solver.poses.clone()
    with pytest.raises(ValueError, match="GPU"):
        solver(res.records.cpu(), res.counts, res.keypoint_records, res.keypoint_counts, res.slot_kp, mc, CAM)
    with pytest.raises(ValueError, match="slot_kp"):
        solver(res.records, res.counts, res.keypoint_records, res.keypoint_counts, res.slot_kp[:, :, :4].contiguous(),
               mc, CAM)
    with pytest.raises(ValueError, match="counts"):
        solver(res.records, res.counts.long(), res.keypoint_records, res.keypoint_counts, res.slot_kp, mc, CAM)
    with pytest.raises(ValueError, match="fx and fy"):
        solver(res.records, res.counts, res.keypoint_records, res.keypoint_counts, res.slot_kp, mc, (0.0, 1, 2, 3))
    with pytest.raises(ValueError, match="min_points"):
        solver(res.records, res.counts, res.keypoint_records, res.keypoint_counts, res.slot_kp, mc, CAM, min_points=5)
    with pytest.raises(ValueError, match="camera"):
        solver(res.records, res.counts, res.keypoint_records, res.keypoint_counts, res.slot_kp, mc, CAM[:3])
    torch.cuda.synchronize()
    assert torch.equal(solver.poses.view(torch.int32), before.view(torch.int32))


def test_captured_graph_of_decode_match_solve():
    tv, oc, mc, pred, _ = _planted(2, 32)
    _, _, _, other, _ = _planted(2, 33)
    dev = torch.device("cuda", 0)
    B, C, H, W = pred.heatmap.shape
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        dec = tv.DeviceKeypointDecoder(B, C, oc.n_keypoints, H, W, 5, 40, oc, dev, poses=True)
        static = {f: getattr(pred, f).clone() for f in ("heatmap", "keypoint_heatmap", "keypoint_affinity", "size")}
        live = type(pred)(**{**{f: None for f in type(pred).__dataclass_fields__}, **static})
        eager = []
        for src in (pred, other):
            for f, t in static.items():
                t.copy_(getattr(src, f))
            dec(live, mc, 0.5, 0.5)
            dec.solve(mc, CAM)
            s.synchronize()
            eager.append(dec.packed.clone())
    torch.cuda.current_stream(dev).wait_stream(s)
    assert not torch.equal(eager[0], eager[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        dec(live, mc, 0.5, 0.5)
        dec.solve(mc, CAM)
    for src, want in ((pred, eager[0]), (other, eager[1]), (pred, eager[0])):
        for f, t in static.items():
            t.copy_(getattr(src, f))
        dec.packed.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dec.packed, want), "replay vs the eager step"


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = (t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t for t in (a, b))
    return torch.equal(a, b)


def test_detector_with_poses():
    import tauv_vision_amd as tv
    from recipe import seeded_u8_frames
    from tauv_vision_amd.weights import seeded_state_dict
    oc = P.four_label_config(tv)
    heights, channels, ds = [2] * 5, [16] * 6, 2
    model = tv.Centernet(tv.DLABackbone(heights, channels, ds), oc, precision="fp16")
    model.load_state_dict(seeded_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()]))
    model = model.cuda().eval()
    mc = tv.ModelConfig(heights, channels, 96, 128, ds, 1.0)
    dev = torch.device("cuda", 0)
    B, K, K_kp, thr = 2, 10, 50, 0.05
    cam = (150.0, 140.0, 64.0, 48.0)
    frames = seeded_u8_frames(B, 96, 128, seed=11).cuda()
    # the default call is what it was: no poses field, the same packed prefix
    base = tv.CenternetDetector(model, B, (96, 128), mc, K, K_kp, dev)
    r0 = base(frames, thr, thr)
    assert type(r0) is tv.CenternetDetections
    with pytest.raises(ValueError, match="go together"):
        base(frames, thr, thr, None, cam)
    det = tv.CenternetDetector(model, B, (96, 128), mc, K, K_kp, dev, poses=True)
    res = det(frames, thr, thr, None, cam)
    assert type(res) is tv.CenternetPoseDetections and res.points is None and res.poses is not None
    n = base.decoder.packed.numel()
    torch.cuda.synchronize()
    assert torch.equal(det.decoder.packed[:n], base.decoder.packed)
    # the detector against its steps: forward_frames -> decoder -> solve, fresh buffers
    pred = model.forward_frames(frames, (96, 128))
    _, C, H, W = pred.heatmap.shape
    steps = tv.DeviceKeypointDecoder(B, C, oc.n_keypoints, H, W, K, K_kp, oc, dev, poses=True)
    want = steps(pred, mc, thr, thr)
    want_poses = steps.solve(mc, cam)
    for f in want._fields:
        assert _same(getattr(res, f), getattr(want, f)), f
    assert _same(res.poses, want_poses)
    host = det.host()
    got = model.detect_keypoints(frames, mc, K, K_kp, thr, thr, camera=cam, poses=True)
    by_matrix = model.detect_keypoints(frames, mc, K, K_kp, thr, thr, poses=True,
                                       M_projection=np.array([[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 0.0]]))
    assert type(got) is tv.CenternetPoseDetections
    for f in host._fields:
        assert _same(getattr(got, f), getattr(host, f)), f
        assert _same(getattr(by_matrix, f), getattr(host, f)), f
    plain = model.detect_keypoints(frames, mc, K, K_kp, thr, thr)
    assert type(plain) is tv.CenternetDetections and _same(plain.records, host.records) and plain.points is None
    without = det(frames, thr, thr)
    assert without.poses is None and det.host().poses is None
    # planted keypoints: overwrite the heads after the forward, rerun decode + match + solve
    heads, truths = P.planted_heads(B, H, W, 4, oc, cam, 41, tz=(0.45, 0.6))
    det(frames, thr, thr, None, cam)
    for f, t in heads.items():
        getattr(det.prediction, f).copy_(t.cuda())
    dec = det.decoder
    r = dec(det.prediction, mc, 0.5, 0.5)
    dec.solve(mc, cam)
    h = dec.host()
    hp = dec.host_poses().numpy()
    assert r.counts.tolist() == [1, 1] and h.n_matched[:, 0].tolist() == [8, 8]
    arrays = tuple(getattr(h, f).numpy() for f in ("records", "counts", "keypoint_records", "keypoint_counts", "slot_kp"))
    ref = _check(arrays, tv.pose_model_points(oc), truths, hp, "planted 24 x 32 in the detector", cam, 96, 128)
    assert ref[:, 0, 12].tolist() == [1, 1] and (hp[:, 1:, 12] == 0).all()


def test_einval_clauses_and_the_empty_batch():
    from tauv_vision_amd import _lib
    table, rng = _table(), np.random.default_rng(24)
    *arrays, _ = P.random_batch(rng, table, PLANAR, 1, 2, 20, [2], FRAME_H, FRAME_W, CAM)
    rc, good = _raw(arrays, table)
    assert rc == 0 and good[0, :, 12].tolist() == [1, 1]
    bad = [dict(rec=None), dict(cnt=None), dict(kp=None), dict(kcnt=None), dict(slot=None), dict(tab=None),
           dict(out=None), dict(B=-1), dict(K=0), dict(K=257), dict(K_kp=0), dict(K_kp=1025), dict(S=0), dict(S=33),
           dict(n_labels=0), dict(min_points=5), dict(min_points=33), dict(in_h=0), dict(in_w=-3), dict(fx=0.0),
           dict(fy=0.0), dict(fx=float("nan")), dict(fy=float("inf"))]
    for o in bad:
        rc, out = _raw(arrays, table, **o)
        assert rc == _lib.TV_EINVAL, o
        assert (out == 7.0).all(), f"{o}: a refused call launched"
        with pytest.raises(ValueError, match="solve_poses"):
            _lib.check(rc, "solve_poses")
    rc, out = _raw(arrays, table, B=0)
    assert rc == 0 and (out == 7.0).all()
