"""Host restatement of the two reference nodes' localisation loops (a helper, not a test):
centernet_node.py:139-178 and yolact_node.py:103-104,135,143,177-193, op for op — a float64
depth image in metres, a uint8 mask, boolean indexing, np.sum / np.mean / np.nanmean, and
F.interpolate itself for the mask mode.

OpenCV is not a dependency of this repository, so `rectangle_fill` restates
cv2.rectangle(img, pt1, pt2, 255, -1) as documented — the filled rectangle between the two
corners, both inclusive, in either corner order, clipped to the image. It is not pinned against
OpenCV itself.

Each function returns one dict per detection: valid, n_pixels, depth_sum, z, x, y, e_x, e_y
(float64; x = y = z = 0 where the node would `continue`). Where the node's own code would raise
(int() of a non-finite corner) the detection is reported invalid with no pixels.
"""
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F


def rectangle_fill(img, pt1, pt2, value):
    """cv2.rectangle(img, pt1, pt2, value, -1): pt = (x, y) integers."""
    H, W = img.shape
    x0, x1 = min(pt1[0], pt2[0]), max(pt1[0], pt2[0])
    y0, y1 = min(pt1[1], pt2[1]), max(pt1[1], pt2[1])
    x0, y0 = max(x0, 0), max(y0, 0)
    x1, y1 = min(x1, W - 1), min(y1, H - 1)
    if x0 <= x1 and y0 <= y1:
        img[y0:y1 + 1, x0:x1 + 1] = value


def _record(valid, n, depth_sum, z, e_x, e_y, fx, fy, cx, cy):
    if not valid:
        return dict(valid=False, n_pixels=n, depth_sum=depth_sum, z=0.0, x=0.0, y=0.0, e_x=e_x, e_y=e_y)
    x = (e_x - cx) * (z / fx)
    y = (e_y - cy) * (z / fy)
    return dict(valid=True, n_pixels=n, depth_sum=depth_sum, z=z, x=x, y=y, e_x=e_x, e_y=e_y)


def centernet_localize(dets, depth_u16, M_projection, box_scale=0.4, min_depth_sum=10, min_z=1):
    """dets: (y, x, h, w) Python floats per detection of one image; depth_u16 [dh, dw] uint16.
    The node's 640 / 360 are its depth image's width / height: here depth_u16's."""
    depth = depth_u16.astype(float) / 1000  # centernet_node.py:84
    dh, dw = depth.shape
    out = []
    for (dy, dx, dhh, dww) in dets:
        e_x = dx * dw
        e_y = dy * dh
        w = dww * dw
        h = dhh * dh
        if not all(math.isfinite(v) for v in (dy, dx, dhh, dww)):
            out.append(_record(False, 0, 0.0, 0.0, e_x, e_y, 1.0, 1.0, 0.0, 0.0))
            continue
        depth_mask = np.zeros(depth.shape, dtype=np.uint8)
        rectangle_fill(depth_mask,
                       (int(e_x - box_scale * w), int(e_y - box_scale * h)),
                       (int(e_x + box_scale * w), int(e_y + box_scale * h)),
                       255)
        sel = depth[(depth_mask > 0) & (depth > 0)]
        n = int(sel.size)
        depth_sum = float(np.sum(sel))
        if n == 0 or depth_sum < min_depth_sum:
            out.append(_record(False, n, depth_sum, 0.0, e_x, e_y, 1.0, 1.0, 0.0, 0.0))
            continue
        z = float(np.mean(sel))
        out.append(_record(not z < min_z, n, depth_sum, z, e_x, e_y, M_projection[0, 0], M_projection[1, 1],
                           M_projection[0, 2], M_projection[1, 2]))
    return out


def yolact_localize(masks, det, box, depth_u16, fx, fy, cx, cy, min_depth_sum=0, min_z=0):
    """masks [n, mh, mw] fp32 torch (CPU), det: n box rows, box [A, 4] fp32 torch (y, x, h, w),
    depth_u16 [H, W] uint16 numpy (the raw image size)."""
    depth = np.where(depth_u16 == 0, np.nan, depth_u16)  # yolact_node.py:103-104
    depth = depth.astype(float) / 1000
    H, W = depth.shape
    out = []
    if len(det) == 0:
        return out
    mask = F.interpolate(masks.unsqueeze(0), (H, W)).squeeze(0)  # yolact_node.py:135
    for detection_i, detection in enumerate(det):
        mask_np = mask[detection_i].detach().cpu().numpy()
        e_x = float(box[detection, 1]) * W
        e_y = float(box[detection, 0]) * H
        picked = np.where(mask_np > 0.5, depth, np.nan)
        n = int(np.count_nonzero(~np.isnan(picked)))
        depth_sum = float(np.nansum(picked))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # mean of an empty slice
            mean_depth = float(np.nanmean(picked))
        if np.isnan(mean_depth) or depth_sum < min_depth_sum:
            out.append(_record(False, n, depth_sum, 0.0, e_x, e_y, 1.0, 1.0, 0.0, 0.0))
            continue
        z = mean_depth
        out.append(_record(not z < min_z, n, depth_sum, z, e_x, e_y, fx, fy, cx, cy))
    return out


def assert_clear_of_thresholds(records, min_depth_sum, min_z, margin=1e-6):
    """The kernel's exact integer sum and this file's float64 sums differ by about 1e-14 relative, so
    the `<` tests can disagree only within ~1e-13 of equality: the inputs of a comparison must keep
    every depth_sum and z at least `margin` away from its threshold."""
    for i, r in enumerate(records):
        if r["n_pixels"] == 0:
            continue
        z = r["depth_sum"] / r["n_pixels"]
        assert abs(r["depth_sum"] - min_depth_sum) >= margin, f"detection {i}: depth_sum {r['depth_sum']} at threshold"
        assert abs(z - min_z) >= margin, f"detection {i}: z {z} at threshold"


def compare_row(got, ref, what=""):
    """got: the 8 fp32 values of one output row; ref: a dict from this file. The comparison rules:
    valid and n_pixels exact; e_x, e_y the float64 reference rounded to fp32; depth_sum, z, x, y
    within one fp32 ulp (rtol 1.2e-7, atol 0) of the float64 reference."""
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == (8,)
    assert bool(got[3] == 1.0) == ref["valid"] and got[3] in (0.0, 1.0), f"{what}: valid {got[3]} vs {ref}"
    assert float(got[4]) == float(ref["n_pixels"]), f"{what}: n_pixels {got[4]} vs {ref}"
    for col, key in ((6, "e_x"), (7, "e_y")):
        want = np.float32(ref[key])
        assert got[col] == want or (np.isnan(got[col]) and np.isnan(want)), f"{what}: {key} {got[col]} vs {want}"
    for col, key in ((5, "depth_sum"), (2, "z"), (0, "x"), (1, "y")):
        want = ref[key]
        assert abs(float(got[col]) - want) <= 1.2e-7 * abs(want), f"{what}: {key} {float(got[col])!r} vs {want!r}"
