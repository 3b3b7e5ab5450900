"""The pose stage on the CPU: the float64 restatement (pnp_ref.py) recovers exact poses and reaches from
its linear start the optimum LM reaches from the truth; the host-side opt-ins of decode.py; and the kernel's
own numerics (csrc/pose_dev.h) through tools/pose_host_check.cpp against the restatement.

Bounds. Exact projections from float64 inputs: 1e-9 (rad, and relative in t) - the LM step tolerance of
1e-12 times a generous 1e3 for the conditioning of the step at these geometries. Inputs rounded to fp32,
the records' type: a pixel moves by at most 4e-5 px, about 5e-7 rad here, asserted at 1e-5 rad and
1e-5 |t|. Linear start against truth start under 0.5 px noise: 1e-7, a tenth of the floor 2^-20 of the
device bar this restatement is the yardstick of."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import pnp_ref as P

MODELS, M_PROJ, (FRAME_H, FRAME_W) = P.load_models()
CAM = (M_PROJ[0, 0], M_PROJ[1, 1], M_PROJ[0, 2], M_PROJ[1, 2])
N_EXACT, N_NOISE = 100, 300
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _fp32_inputs(obj, uv):
    """The inputs as the device sees them: fp32 model points, pixels from fp32 normalised coordinates."""
    u = (uv[:, 0] / FRAME_W).astype(np.float32).astype(np.float64) * FRAME_W
    v = (uv[:, 1] / FRAME_H).astype(np.float32).astype(np.float64) * FRAME_H
    return obj.astype(np.float32).astype(np.float64), np.stack([u, v], axis=1)


def _errors(row, R, t):
    return P.geodesic(row[0:9].reshape(3, 3), R), float(np.linalg.norm(row[9:12] - t) / np.linalg.norm(t))


@pytest.mark.parametrize("name", ["eight", "seven"])
def test_exact_projections_give_the_true_pose(name):
    obj, rng = MODELS[name], np.random.default_rng(11)
    worst64, worst32, iters = np.zeros(2), np.zeros(2), 0
    for _ in range(N_EXACT):
        R, t = P.random_pose(rng)
        uv, z = P.project(R, t, obj, CAM)
        assert (z > 0).all()
        row = P.solve(obj, uv, CAM)
        assert row[12] == 1 and row[13] == len(obj)
        worst64 = np.maximum(worst64, _errors(row, R, t))
        iters = max(iters, int(row[15]))
        row32 = P.solve(*_fp32_inputs(obj, uv), CAM)
        assert row32[12] == 1
        worst32 = np.maximum(worst32, _errors(row32, R, t))
    print(f"{name}: float64 inputs worst {worst64}, fp32 inputs worst {worst32}, at most {iters} iterations")
    assert (worst64 <= 1e-9).all()
    assert (worst32 <= 1e-5).all()


@pytest.mark.parametrize("name", ["eight", "seven"])
def test_noisy_keypoints_linear_start_reaches_the_truth_started_optimum(name):
    obj, rng = MODELS[name], np.random.default_rng(12)
    worst, iters = np.zeros(2), 0
    for i in range(N_NOISE):
        R, t = P.random_pose(rng)
        uv, _ = P.project(R, t, obj, CAM)
        uv = uv + rng.normal(scale=0.5, size=uv.shape)
        a, b = P.solve(obj, uv, CAM), P.solve(obj, uv, CAM, start=(R, t))
        assert a[12] == 1 and b[12] == 1, i
        e = P.pose_errors(a, b)
        assert e[0] <= 1e-7 and e[1] <= 1e-7, (i, e, a[14], b[14])
        worst = np.maximum(worst, e[:2])
        iters = max(iters, int(a[15]))
    print(f"{name}: linear start against truth start worst {worst}, at most {iters} iterations")


def test_planar_octagon_exact_and_noisy():
    obj, rng = P.octagon(), np.random.default_rng(13)
    worst, other = np.zeros(2), 0
    for i in range(N_EXACT):
        R, t = P.tilted_pose(rng)
        uv, z = P.project(R, t, obj, CAM)
        assert (z > 0).all()
        row = P.solve(obj, uv, CAM)
        assert row[12] == 1
        worst = np.maximum(worst, _errors(row, R, t))
        # with noise: a stationary point, at the truth-started cost or the mirrored solution; never the pose
        uvn = uv + rng.normal(scale=0.5, size=uv.shape)
        a, b = P.solve(obj, uvn, CAM), P.solve(obj, uvn, CAM, start=(R, t))
        assert a[12] == 1 and b[12] == 1, i
        JtJ, Jtr, cost = P.normal_equations(a[0:9].reshape(3, 3), a[9:12], obj, uvn, CAM)
        # |J^T r| <= |J^T J| |step|, and LM stopped on a step of 1e-12 (1 + |t|): 1e-9 leaves a factor of 400
        assert np.linalg.norm(Jtr) <= 1e-9 * np.linalg.norm(JtJ), (i, np.linalg.norm(Jtr) / np.linalg.norm(JtJ))
        if not cost <= (b[14] ** 2 * len(obj)) * (1 + 1e-9):
            other += 1
            c = P.solve(obj, uvn, CAM, start=P.mirrored_pose(R, t, obj))
            assert c[12] == 1 and max(P.pose_errors(a, c)[:2]) <= 1e-7, (i, a[14], b[14], c[14])
    print(f"octagon: exact worst {worst}; {other} of {N_EXACT} noisy cases ended in the mirrored minimum")
    assert (worst <= 1e-9).all()


def test_degenerate_inputs_are_invalid():
    obj, rng = MODELS["eight"], np.random.default_rng(14)
    R, t = P.random_pose(rng)
    uv, _ = P.project(R, t, obj, CAM)
    bad = uv.copy()
    bad[3] = np.nan
    behind = P.project(R, t * np.array([1, 1, -1.0]), obj, CAM)[0]
    for o, i in ((obj, bad), (obj, np.tile(uv[:1], (8, 1))), (np.tile(obj[:1], (8, 1)), uv), (obj[:5], uv[:5])):
        row = P.solve(o, i, CAM)
        assert row[12] == 0 and row[13] == len(o) and np.isnan(row[0:12]).all() and np.isnan(row[14])
    row = P.solve(obj, behind, CAM)  # whatever it ends at, a valid row has every point in front
    if row[12] == 1:
        assert (P.project(row[0:9].reshape(3, 3), row[9:12], obj, CAM)[1] > 0).all()


def test_pose_model_points_and_the_host_opt_ins():
    import tauv_vision_amd as tv
    import importlib
    D = importlib.import_module("tauv_vision_amd.decode")  # (the package attribute `decode` is the function)
    oc = P.four_label_config(tv)
    table = tv.pose_model_points(oc)
    assert table.dtype == np.float32 and table.shape == (4, 8, 3)
    np.testing.assert_array_equal(table[0], MODELS["eight"].astype(np.float32))
    np.testing.assert_array_equal(table[1, :7], MODELS["seven"].astype(np.float32))
    assert np.isnan(table[1, 7]).all() and np.isnan(table[3, 1:]).all() and not np.isnan(table[3, 0]).any()
    A = tv.AngleConfig(False, None)
    mixed = tv.ObjectConfigSet([tv.ObjectConfig("a", A, A, A, False, False, None),
                                tv.ObjectConfig("b", A, A, A, False, True, [(1.0, 2.0, 3.0)])])
    t2 = tv.pose_model_points(mixed)
    assert t2.shape == (2, 1, 3) and np.isnan(t2[0]).all() and t2[1, 0].tolist() == [1.0, 2.0, 3.0]

    # records of one image: an 8-point object with all keypoints, a 7-point object with five
    rng = np.random.default_rng(15)
    poses_true = [P.random_pose(rng), P.random_pose(rng)]
    uv0, _ = P.project(*poses_true[0], MODELS["eight"], CAM)
    uv1, _ = P.project(*poses_true[1], MODELS["seven"], CAM)
    rec = P.make_records([[(0, {s: tuple(uv0[s]) for s in range(8)}), (1, {s: tuple(uv1[s]) for s in range(5)})]],
                         3, 20, 8, FRAME_H, FRAME_W)
    mc = tv.ModelConfig([2] * 5, [16] * 6, FRAME_H, FRAME_W, 2, 1.0)
    poses = P.solve_poses(*rec, table, FRAME_H, FRAME_W, CAM).astype(np.float32)
    assert poses[0, :, 12].tolist() == [1, 0, 0]
    dets = tv.keypoint_detections_from_records(rec[0], rec[1], rec[2], rec[4], False, mc, oc, M_PROJ, poses=poses)
    assert len(dets) == 1 and len(dets[0]) == 2 and dets[0][1].cam_t_object is None
    R, t = dets[0][0].cam_t_object
    assert R.dtype == np.float64 and R.shape == (3, 3) and t.dtype == np.float64 and t.shape == (3, 1)
    np.testing.assert_array_equal(R, poses[0, 0, 0:9].astype(np.float64).reshape(3, 3))
    np.testing.assert_array_equal(t[:, 0], poses[0, 0, 9:12].astype(np.float64))
    assert P.geodesic(R, poses_true[0][0]) <= 1e-5
    assert [k is not None for k in dets[0][1].keypoints] == [True] * 5 + [False] * 2
    with pytest.raises(ValueError, match="poses must be"):
        tv.keypoint_detections_from_records(rec[0], rec[1], rec[2], rec[4], False, mc, oc, M_PROJ, poses=poses[:, :2])

    # the defaults are what they were: the host _solve_poses, which needs OpenCV from six keypoints on
    try:
        import cv2  # noqa: F401
        has_cv2 = True
    except ImportError:
        has_cv2 = False
    if not has_cv2:
        with pytest.raises(RuntimeError, match="solvePnP needs OpenCV"):
            tv.keypoint_detections_from_records(rec[0], rec[1], rec[2], rec[4], False, mc, oc, M_PROJ)
    few = P.make_records([[(1, {s: tuple(uv1[s]) for s in range(5)})]], 3, 20, 8, FRAME_H, FRAME_W)
    d5 = tv.keypoint_detections_from_records(few[0], few[1], few[2], few[4], False, mc, oc, M_PROJ)
    assert d5[0][0].cam_t_object is None and d5[0][0].label == 1
    sig = inspect.signature(tv.decode_keypoints)
    assert sig.parameters["pose"].default == "cv2" and list(sig.parameters)[-1] == "pose"
    assert inspect.signature(tv.keypoint_detections_from_records).parameters["poses"].default is None
    with pytest.raises(ValueError, match="pose must be"):
        tv.decode_keypoints(None, mc, oc, M_PROJ, 3, 20, 0.5, 0.5, 0.0, pose="opencv")
    assert D.camera_of(np.array([[732, 0, 320], [0, 731, 180], [0, 0, 0]])) == (732.0, 731.0, 320.0, 180.0)
    for name in ("DevicePoseSolver", "decode_keypoint_poses", "CenternetPoseDetections", "pose_model_points"):
        assert hasattr(tv, name), name
    assert tv.CenternetPoseDetections._fields == tv.CenternetDetections._fields + ("poses",)


def test_the_entry_is_declared_bound_and_built():
    from tauv_vision_amd import _lib
    text = open(os.path.join(ROOT, "include", "tauv_vision_amd.h")).read()
    decl = re.search(r"int tv_solve_poses\(([^;]*)\);", text)
    assert decl and "tv_solve_poses" in _lib.EXPORTS
    assert len(decl.group(1).split(",")) == len(_lib.EXPORTS["tv_solve_poses"][0]) == 20
    mk = open(os.path.join(ROOT, "tauv-vision_amd", "Makefile")).read()
    assert "csrc/pose.hip" in mk and "csrc/pose_dev.h" in mk


def _host_cases():
    """(obj, img, truth or None) as the device would see them: the three models exact and with noise, then
    the degenerate rows of the GPU test."""
    rng, cases = np.random.default_rng(16), []
    for obj, planar in ((MODELS["eight"], False), (MODELS["seven"], False), (P.octagon(), True)):
        for i in range(24):
            R, t = P.tilted_pose(rng) if planar else P.random_pose(rng)
            uv, _ = P.project(R, t, obj, CAM)
            if i % 2:
                uv = uv + rng.normal(scale=0.5, size=uv.shape)
            cases.append((*_fp32_inputs(obj, uv), (R, t)))
    obj = MODELS["eight"].astype(np.float32).astype(np.float64)
    uv = cases[0][1]
    bad = uv.copy()
    bad[3] = np.nan
    cases += [(obj, bad, None), (obj, np.tile(uv[:1], (8, 1)), None), (np.tile(obj[:1], (8, 1)), uv, None),
              (obj[:5], uv[:5], None), (obj[:6], uv[:6], cases[0][2])]
    return cases


def test_the_kernels_numerics_on_the_host(tmp_path):
    """tools/pose_host_check.cpp (pose_dev.h compiled for the host, no sanitizer) against the restatement
    at the device bar."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "pose_host_check")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-x", "hip",
                    os.path.join(ROOT, "tools", "pose_host_check.cpp"), "-o", exe], check=True)
    cases = _host_cases()
    text = ""
    for obj, img, _ in cases:
        text += f"{len(obj)} " + " ".join(repr(float(c)) for c in CAM) + " 6\n"
        text += "".join(" ".join(repr(float(a)) for a in (*X, *q)) + "\n" for X, q in zip(obj, img))
    path = tmp_path / "cases.txt"
    path.write_text(text)
    by_file = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout
    by_stdin = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    assert by_file == by_stdin
    got = np.array([[float(x) for x in line.split()] for line in by_file.strip().split("\n")])
    assert got.shape == (len(cases), 16)
    worst = np.zeros(3)
    for i, ((obj, img, truth), row) in enumerate(zip(cases, got)):
        ref = P.solve(obj, img, CAM)
        assert row[12] == ref[12] and row[13] == ref[13] and (np.isnan(row) == np.isnan(ref)).all(), (i, row, ref)
        if ref[12] != 1:
            continue
        bar = np.full(3, P.FLOOR)
        if truth is not None:
            alt = P.solve(obj, img, CAM, start=truth)
            bar = np.maximum(bar, 4 * np.asarray(P.pose_errors(ref.astype(np.float32), alt.astype(np.float32))))
        e = np.asarray(P.pose_errors(row, ref.astype(np.float32)))
        assert (e <= bar).all(), (i, e, bar)
        worst = np.maximum(worst, e)
    print(f"pose_host_check against pnp_ref: worst angle / |dt|/|t| / rms {worst}, floor {P.FLOOR}")
    assert got[-5:-1, 12].tolist() == [0, 0, 0, 0] and got[-1, 12] == 1
