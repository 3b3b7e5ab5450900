"""Test infrastructure of the pose stage (tv_solve_poses, csrc/pose.hip): a float64 numpy restatement of
its contract (include/tauv_vision_amd.h), the synthetic scenes the tests share, and the error measures.

The pose of n >= min_points correspondences (object point X_i, pixel (u_i, v_i)) is the (R, t) that
minimises sum_i (fx Xc/Zc + cx - u_i)^2 + (fy Yc/Zc + cy - v_i)^2, Xc = R X_i + t. It is found from a linear
start (Hartley-normalised 12-parameter DLT, or a homography and its decomposition when the object points
are coplanar; none when all object points or all pixels are equal) polished by Levenberg-Marquardt on a
rotation-vector increment (R <- exp([w]x) R) and t, run
here to a step of 1e-12 (1 + |t|) or 50 iterations. numpy's eigh stands where the kernel has its Jacobi
routine. OpenCV is not part of this stack: nothing here claims its iteration count, its termination or its
choice between the two minima of a planar target."""
import json
import os

import numpy as np

MAX_ITER = 50
MAX_TRIES = 12          # the damping ladder of one iteration
STEP_TOL = 1e-12
PLANAR_RATIO = 1e-6     # smallest / middle eigenvalue of the centred scatter (OpenCV's 1e-3 on singular values)
COLS = 16
FLOOR = 2.0 ** -20      # the floor of the device bar

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_models.json")


def load_models():
    """(models: name -> float64 [n, 3], M_projection float64 [3, 3], (frame_h, frame_w)) of the fixture."""
    with open(_GOLDEN) as f:
        data = json.load(f)
    return ({k: np.asarray(v, dtype=np.float64) for k, v in data["models"].items()},
            np.asarray(data["M_projection"], dtype=np.float64), tuple(data["frame_hw"]))


def octagon(radius=0.12):
    """The planar 8-point model of the tests: a regular octagon in the plane y = 0.02."""
    a = np.arange(8) * (np.pi / 4) + 0.2
    return np.stack([radius * np.cos(a), np.full(8, 0.02), radius * np.sin(a)], axis=1)


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    """Rodrigues' formula."""
    th = float(np.sqrt(w @ w))
    K = skew(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def geodesic(Ra, Rb):
    """The angle of Ra Rb^T in radians, from the skew part and the trace (accurate near 0 and near pi)."""
    D = np.asarray(Ra, dtype=np.float64) @ np.asarray(Rb, dtype=np.float64).T
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return float(np.arctan2(s, 0.5 * (np.trace(D) - 1.0)))


def project(R, t, obj, cam):
    fx, fy, cx, cy = cam
    Xc = obj @ R.T + t
    return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], axis=1), Xc[:, 2]


def cost_of(R, t, obj, img, cam):
    uv, _ = project(R, t, obj, cam)
    return float(((uv - img) ** 2).sum())


def normal_equations(R, t, obj, img, cam):
    """J^T J [6, 6], J^T r [6] and the cost at (R, t), for the increment (w, dt): R <- exp([w]x) R, t <- t + dt."""
    fx, fy, cx, cy = cam
    JtJ, Jtr, cost = np.zeros((6, 6)), np.zeros(6), 0.0
    for X, (u, v) in zip(obj, img):
        Y = R @ X
        x, y, z = Y + t
        r = np.array([fx * x / z + cx - u, fy * y / z + cy - v])
        Jp = np.array([[fx / z, 0.0, -fx * x / (z * z)], [0.0, fy / z, -fy * y / (z * z)]])
        J = np.concatenate([-Jp @ skew(Y), Jp], axis=1)
        JtJ += J.T @ J
        Jtr += J.T @ r
        cost += float(r @ r)
    return JtJ, Jtr, cost


def nearest_rotation(M):
    """(R, scale): the rotation nearest M in the Frobenius norm and the matching scale, from the
    eigenvectors of M^T M (the two largest singular pairs; the third axis by cross products, so det = +1)."""
    w, V = np.linalg.eigh(M.T @ M)
    v1, v2 = V[:, 2], V[:, 1]
    s1, s2 = np.sqrt(w[2]), np.sqrt(max(w[1], 0.0))
    u1, u2 = M @ v1 / s1, M @ v2 / s2
    u1 = u1 / np.sqrt(u1 @ u1)
    u2 = u2 - (u1 @ u2) * u1  # orthogonal already unless the second singular value is at rounding level
    u2 = u2 / np.sqrt(u2 @ u2)
    u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
    R = np.outer(u1, v1) + np.outer(u2, v2) + np.outer(u3, v3)
    s3 = float(u3 @ M @ v3)
    return R, (s1 + s2 + s3) / 3.0


def initial_pose(obj, xn):
    """The linear start (R, t) from object points [n, 3] and normalised image points [n, 2], or None when
    the object points have no extent."""
    n = len(obj)
    m = obj.mean(axis=0)
    Xc = obj - m
    w, E = np.linalg.eigh(Xc.T @ Xc)
    if not np.isfinite(w).all() or not w[2] > 0.0:
        return None
    if w[0] < PLANAR_RATIO * w[1]:
        ea, eb = E[:, 2], E[:, 1]
        Rp = np.stack([ea, eb, np.cross(ea, eb)], axis=1)
        sc = np.sqrt(2.0 * n / (w[1] + w[2]))
        a, b = sc * (Xc @ ea), sc * (Xc @ eb)
        A = np.zeros((2 * n, 9))
        for i in range(n):
            x, y = xn[i]
            A[2 * i] = [a[i], b[i], 1, 0, 0, 0, -x * a[i], -x * b[i], -x]
            A[2 * i + 1] = [0, 0, 0, a[i], b[i], 1, -y * a[i], -y * b[i], -y]
        _, V = np.linalg.eigh(A.T @ A)
        H = V[:, 0].reshape(3, 3)
        if np.mean(H[2, 0] * a + H[2, 1] * b + H[2, 2]) < 0:
            H = -H
        h1, h2 = H[:, 0], H[:, 1]
        lam = 0.5 * (np.sqrt(h1 @ h1) + np.sqrt(h2 @ h2))
        if not lam > 0.0:
            return None
        M = np.stack([h1 / lam, h2 / lam, np.cross(h1, h2) / (lam * lam)], axis=1)
        Rh, _ = nearest_rotation(M)
        R = Rh @ Rp.T
        return R, H[:, 2] / (lam * sc) - R @ m
    sc = np.sqrt(3.0 * n / w.sum())
    Xs = sc * Xc
    A = np.zeros((2 * n, 12))
    for i in range(n):
        x, y = xn[i]
        X = np.append(Xs[i], 1.0)
        A[2 * i, 0:4], A[2 * i, 8:12] = X, -x * X
        A[2 * i + 1, 4:8], A[2 * i + 1, 8:12] = X, -y * X
    _, V = np.linalg.eigh(A.T @ A)
    P = V[:, 0].reshape(3, 4)
    if np.mean(Xs @ P[2, :3] + P[2, 3]) < 0:
        P = -P
    R, scale = nearest_rotation(P[:, :3])
    if not scale > 0.0:
        return None
    return R, P[:, 3] / (scale * sc) - R @ m


def refine(obj, img, cam, R, t, max_iter=MAX_ITER):
    """Levenberg-Marquardt from (R, t): (R, t, cost, iterations, converged)."""
    cost = cost_of(R, t, obj, img, cam)
    lam, iters = 1e-3, 0
    if not np.isfinite(cost):
        return R, t, cost, 0, False
    while iters < max_iter:
        JtJ, Jtr, _ = normal_equations(R, t, obj, img, cam)
        iters += 1
        moved = False
        for _ in range(MAX_TRIES):
            A = JtJ + lam * np.diag(np.diag(JtJ))
            try:
                L = np.linalg.cholesky(A)
                d = -np.linalg.solve(L.T, np.linalg.solve(L, Jtr))
            except np.linalg.LinAlgError:
                lam = min(lam * 10.0, 1e12)
                continue
            R2, t2 = exp_so3(d[:3]) @ R, t + d[3:]
            c2 = cost_of(R2, t2, obj, img, cam)
            small = np.sqrt(d @ d) <= STEP_TOL * (1.0 + np.sqrt(t @ t))
            if np.isfinite(c2) and c2 <= cost:
                R, t, cost, moved = R2, t2, c2, True
                lam = max(lam * 0.1, 1e-12)
            if small:
                return R, t, cost, iters, True
            if moved:
                break
            lam = min(lam * 10.0, 1e12)
        if not moved:  # no damping of the ladder lowers the cost: a minimum to rounding
            return R, t, cost, iters, True
    return R, t, cost, iters, False


def solve(obj, img, cam, min_points=6, start=None):
    """One detection: the 16 columns (float64). start = (R, t) replaces the linear start."""
    row = np.full(COLS, np.nan)
    n = len(obj)
    row[12], row[13], row[15] = 0.0, float(n), 0.0
    if n < min_points:
        return row
    obj, img = np.asarray(obj, dtype=np.float64), np.asarray(img, dtype=np.float64)
    fx, fy, cx, cy = cam
    with np.errstate(all="ignore"):
        if start is None:
            xn = np.stack([(img[:, 0] - cx) / fx, (img[:, 1] - cy) / fy], axis=1)
            if not (np.isfinite(obj).all() and np.isfinite(xn).all()):
                return row
            if (obj == obj[0]).all() or (img == img[0]).all():  # no extent in the model or in the picture
                return row
            start = initial_pose(obj, xn)
            if start is None or not (np.isfinite(start[0]).all() and np.isfinite(start[1]).all()):
                return row
        R, t, cost, iters, ok = refine(obj, img, cam, np.asarray(start[0], dtype=np.float64),
                                       np.asarray(start[1], dtype=np.float64).reshape(3))
        row[15] = float(iters)
        _, z = project(R, t, obj, cam)
        if not ok or not np.isfinite(R).all() or not np.isfinite(t).all() or not np.isfinite(cost) or not (z > 0).all():
            return row
    row[0:9], row[9:12], row[12], row[14] = R.reshape(9), t, 1.0, np.sqrt(cost / n)
    return row


def gather(records, counts, kp_records, kp_counts, slot_kp, model_points, in_h, in_w, b, d):
    """The correspondences of detection (b, d) as the contract lists them: (obj [n, 3], img [n, 2]) float64."""
    K_kp = kp_records.shape[1]
    n_labels, S, _ = model_points.shape
    obj, img = [], []
    if d < min(max(int(counts[b]), 0), records.shape[1]):
        label = int(records[b, d, 0])
        if 0 <= label < n_labels:
            nk = min(max(int(kp_counts[b]), 0), K_kp)
            for s in range(S):
                X = model_points[label, s]
                k = int(slot_kp[b, d, s])
                if np.isnan(X).any() or not 0 <= k < nk:
                    continue
                obj.append(X.astype(np.float64))
                img.append([float(kp_records[b, k, 3]) * in_w, float(kp_records[b, k, 2]) * in_h])
    return np.asarray(obj, dtype=np.float64).reshape(-1, 3), np.asarray(img, dtype=np.float64).reshape(-1, 2)


def solve_poses(records, counts, kp_records, kp_counts, slot_kp, model_points, in_h, in_w, cam, min_points=6,
                starts=None):
    """poses [B, K, 16] float64 of the contract; starts: {(b, d): (R, t)} replaces the linear start there."""
    B, K = records.shape[:2]
    out = np.full((B, K, COLS), np.nan)
    for b in range(B):
        for d in range(K):
            obj, img = gather(records, counts, kp_records, kp_counts, slot_kp, model_points, in_h, in_w, b, d)
            out[b, d] = solve(obj, img, cam, min_points, None if starts is None else starts.get((b, d)))
    return out


# ---- scenes --------------------------------------------------------------------------------------

def random_rotation(rng, max_angle=0.999 * np.pi):
    axis = rng.normal(size=3)
    axis /= np.sqrt(axis @ axis)
    return exp_so3(axis * rng.uniform(0.0, max_angle))


def random_pose(rng, tz=(0.6, 1.5)):
    """The ranges of the tests: any rotation up to 0.999 pi, t_z in tz metres, t_x +-0.5, t_y +-0.3."""
    return random_rotation(rng), np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(*tz)])


def tilted_pose(rng, max_tilt_deg=70.0):
    """A pose under which the plane y = const of the octagon faces the camera within max_tilt: the normal
    (object y) is turned onto -z of the camera, tilted by up to max_tilt, then spun about the normal."""
    base = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])  # object y -> camera -z
    ax = rng.uniform(0.0, 2 * np.pi)
    tilt = exp_so3(np.array([np.cos(ax), np.sin(ax), 0.0]) * np.deg2rad(rng.uniform(0.0, max_tilt_deg)))
    spin = exp_so3(np.array([0.0, 1.0, 0.0]) * rng.uniform(0.0, 2 * np.pi))
    return tilt @ base @ spin, np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(0.6, 1.5)])


def mirrored_pose(R, t, obj):
    """The other pose of a planar target that explains the same picture under weak perspective: the plane's
    normal reflected about the line of sight to the centroid."""
    m = obj.mean(axis=0)
    Xc = obj - m
    _, E = np.linalg.eigh(Xc.T @ Xc)
    c = R @ m + t
    los = c / np.sqrt(c @ c)
    R2 = exp_so3(los * np.pi) @ R @ exp_so3(E[:, 0] * np.pi)
    return R2, c - R2 @ m


def pose_errors(row, ref_row):
    """(geodesic angle, |dt| / |t|, relative rms difference) of two valid rows."""
    Ra, Rb = np.asarray(row[0:9], dtype=np.float64).reshape(3, 3), np.asarray(ref_row[0:9], dtype=np.float64).reshape(3, 3)
    ta, tb = np.asarray(row[9:12], dtype=np.float64), np.asarray(ref_row[9:12], dtype=np.float64)
    return (geodesic(Ra, Rb), float(np.sqrt(((ta - tb) ** 2).sum()) / np.sqrt((tb ** 2).sum())),
            float(abs(row[14] - ref_row[14]) / max(abs(ref_row[14]), 1e-300)))


def make_records(dets, K, K_kp, S, in_h, in_w):
    """Pack hand-made detections of one batch into the arrays of the contract. dets[b]: a list of
    (label, {slot: (u, v)}) in object order; keypoints are numbered in the order they are listed. Returns
    float32 records [B, K, 10], int32 counts [B], float32 kp_records [B, K_kp, 10], int32 kp_counts [B],
    int32 slot_kp [B, K, S]. The keypoint columns hold y = v / in_h, x = u / in_w rounded to fp32."""
    B = len(dets)
    rec = np.zeros((B, K, 10), dtype=np.float32)
    kp = np.zeros((B, K_kp, 10), dtype=np.float32)
    counts, kcounts = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    slot = np.full((B, K, S), -1, dtype=np.int32)
    for b, objs in enumerate(dets):
        k = 0
        for d, (label, pts) in enumerate(objs):
            rec[b, d, 0], rec[b, d, 1] = label, 0.9
            for s, (u, v) in sorted(pts.items()):
                kp[b, k, 0], kp[b, k, 1], kp[b, k, 2], kp[b, k, 3] = s, 0.8, v / in_h, u / in_w
                slot[b, d, s] = k
                k += 1
        counts[b], kcounts[b] = len(objs), k
    return rec, counts, kp, kcounts, slot


def four_label_config(tv):
    """The four labels of the tests as an ObjectConfigSet of the package `tv`: the fixture's 8- and 7-point
    models, the planar octagon and a one-keypoint model; max_slots = 8."""
    models, _, _ = load_models()
    A = tv.AngleConfig(False, None)
    kps = [models["eight"], models["seven"], octagon(), np.array([[0.0, 0.0, 0.0]])]
    return tv.ObjectConfigSet([tv.ObjectConfig(f"o{i}", A, A, A, False, True, [tuple(float(v) for v in p) for p in k])
                               for i, k in enumerate(kps)])


def model_table(models):
    """float32 [n_labels, max_slots, 3] with NaN rows past a model's points (pose_model_points' layout)."""
    S = max(len(m) for m in models)
    out = np.full((len(models), S, 3), np.nan, dtype=np.float32)
    for i, m in enumerate(models):
        out[i, :len(m)] = m
    return out


def random_batch(rng, table, planar_labels, B, K, K_kp, counts, in_h, in_w, cam, noise=0.5, drop=None):
    """A batch of detections with drawn poses: every object of image b < counts[b] gets a label with at
    least six points, a pose from the tests' ranges (tilted_pose for a planar label), its keypoints
    projected (+ Gaussian noise in pixels on odd objects) and matched in slot order. drop: {(b, d): slots
    left unmatched}. Returns (records, counts, kp_records, kp_counts, slot_kp, truths {(b, d): (R, t)})."""
    labels = [l for l in range(table.shape[0]) if (~np.isnan(table[l, :, 0])).sum() >= 6]
    dets, truths = [], {}
    for b in range(B):
        objs = []
        for d in range(int(counts[b])):
            l = labels[int(rng.integers(len(labels)))]
            obj = table[l][~np.isnan(table[l, :, 0])].astype(np.float64)
            R, t = tilted_pose(rng) if l in planar_labels else random_pose(rng)
            uv, _ = project(R, t, obj, cam)
            if d % 2:
                uv = uv + rng.normal(scale=noise, size=uv.shape)
            gone = (drop or {}).get((b, d), ())
            objs.append((l, {s: tuple(uv[s]) for s in range(len(obj)) if s not in gone}))
            truths[(b, d)] = (R, t)
        dets.append(objs)
    return (*make_records(dets, K, K_kp, table.shape[1], in_h, in_w), truths)


def reference_and_bars(arrays, table, in_h, in_w, cam, truths, min_points=6):
    """(poses [B, K, 16] float64 of the restatement from the linear start, bars [B, K, 3]): the device bar
    max(4 e_ref, 2^-20) per measure of pose_errors, e_ref the distance between the restatement's linearly
    started and truth-started runs after rounding to the fp32 output (the floor where a row has no truth)."""
    ref = solve_poses(*arrays, table, in_h, in_w, cam, min_points)
    alt = solve_poses(*arrays, table, in_h, in_w, cam, min_points, starts=truths)
    bars = np.full(ref.shape[:2] + (3,), FLOOR)
    for (b, d) in truths:
        if ref[b, d, 12] == 1 and alt[b, d, 12] == 1:
            e = pose_errors(ref[b, d].astype(np.float32), alt[b, d].astype(np.float32))
            bars[b, d] = np.maximum(4.0 * np.asarray(e), FLOOR)
    return ref, bars


def assert_poses(got, ref, bars, what=""):
    """valid, n and the NaN pattern exactly; R, t and rms of the valid rows within the bars. Returns the
    largest (angle, |dt|/|t|, rms) errors seen."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    np.testing.assert_array_equal(got[..., 12], ref[..., 12], err_msg=f"{what}: valid")
    np.testing.assert_array_equal(got[..., 13], ref[..., 13], err_msg=f"{what}: n")
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=f"{what}: NaN pattern")
    worst = np.zeros(3)
    for b, d in zip(*np.nonzero(ref[..., 12] == 1)):
        e = np.asarray(pose_errors(got[b, d], ref[b, d].astype(np.float32)))
        assert (e <= bars[b, d]).all(), f"{what}: row ({b}, {d}) errors {e} over the bars {bars[b, d]}"
        worst = np.maximum(worst, e)
    return worst


def planted_heads(B, H, W, ratio, object_config, cam, seed, label=0, tz=(0.5, 0.7)):
    """Head tensors (CPU, the reference's Prediction layout) with one planted object of `label` per image:
    background logit -8, the object's peak at the cell of its projected centroid and one peak per keypoint
    at the cell nearest its projection (tv_decode mode 1 reports cell * ratio as the pixel), distinct
    logits so that no two scores tie. Returns (dict of tensors, truths {(b, 0): (R, t)})."""
    import torch
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    C, C_kp = object_config.n_labels, object_config.n_keypoints
    heat = torch.full((B, C, H, W), -8.0)
    kheat = torch.full((B, C_kp, H, W), -8.0)
    obj = np.asarray(object_config.configs[label].keypoints, dtype=np.float64)
    truths = {}
    for b in range(B):
        while True:
            R = random_rotation(rng)
            t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.08, 0.08), rng.uniform(*tz)])
            uv, z = project(R, t, obj, cam)
            cells = np.rint(uv / ratio).astype(int)
            if (z > 0).all() and (cells[:, 0] >= 1).all() and (cells[:, 0] < W - 1).all() and \
                    (cells[:, 1] >= 1).all() and (cells[:, 1] < H - 1).all():
                break
        c = np.rint(uv.mean(axis=0) / ratio).astype(int)
        heat[b, label, c[1], c[0]] = 3.0
        for s, (ix, iy) in enumerate(cells):
            kheat[b, object_config.encode_keypoint_index(label, s), iy, ix] = 2.0 + 0.1 * s
        truths[(b, 0)] = (R, t)
    heads = dict(heatmap=heat, keypoint_heatmap=kheat, keypoint_affinity=torch.randn((B, C_kp, 2, H, W), generator=g),
                 size=torch.rand((B, H, W, 2), generator=g), offset=torch.zeros((B, H, W, 2)))
    return heads, truths
