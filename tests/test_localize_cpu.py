"""Known answers for tests/localize_ref.py (the host restatement of the nodes' localisation loops
that the GPU tests compare against) on a 4 x 6 depth image worked by hand, and the argument
validation of the Python entry points that needs no GPU."""
import numpy as np
import pytest
import torch

import localize_ref as ref
from tauv_vision_amd import localize as loc
from tauv_vision_amd.decode import Detection

# millimetres; rows 2-3 x columns 0-3 are all zero
DEPTH = np.array([[1000, 2000, 0, 4000, 5000, 6000],
                  [1500, 0, 3500, 4500, 0, 6500],
                  [0, 0, 0, 0, 7000, 8000],
                  [0, 0, 0, 0, 9000, 10000]], dtype=np.uint16)
# fx = 2, fy = 4, cx = 2.5, cy = 2
M = np.array([[2.0, 0.0, 2.5], [0.0, 4.0, 2.0], [0.0, 0.0, 0.0]])


def test_interior_box():
    # e_x = 3, W = 3: columns int(1.8) = 1 .. int(4.2) = 4; e_y = 1, H = 1: rows int(0.6) = 0 .. int(1.4) = 1
    # positive depth there: 2000 4000 5000 / 3500 4500 -> 5 pixels, 19 m, z = 3.8
    r, = ref.centernet_localize([(0.25, 0.5, 0.25, 0.5)], DEPTH, M)
    assert r["valid"] and r["n_pixels"] == 5
    assert r["depth_sum"] == pytest.approx(19.0, rel=1e-14)
    assert r["z"] == pytest.approx(3.8, rel=1e-14)
    assert r["e_x"] == 3.0 and r["e_y"] == 1.0
    assert r["x"] == pytest.approx(0.5 * 1.9, rel=1e-14)
    assert r["y"] == pytest.approx(-0.95, rel=1e-14)


def test_box_off_the_left_edge_selects_column_0():
    # e_x = -1.5, 0.4 W = 0.8: corners int(-2.3) = -2 and int(-0.7) = 0 (truncation, not floor) -> column 0
    # rows int(0.4) = 0 .. int(3.6) = 3; column 0 holds 1000, 1500, 0, 0 -> 2 pixels, 2.5 m
    det = (0.5, -0.25, 1.0, 1.0 / 3.0)
    assert -1.5 + 0.4 * ((1.0 / 3.0) * 6) == pytest.approx(-0.7)
    r, = ref.centernet_localize([det], DEPTH, M, min_depth_sum=1)
    assert r["valid"] and r["n_pixels"] == 2
    assert r["depth_sum"] == pytest.approx(2.5, rel=1e-14) and r["z"] == pytest.approx(1.25, rel=1e-14)
    assert r["x"] == pytest.approx(-4.0 * 0.625, rel=1e-14) and r["y"] == 0.0
    # the node's thresholds: 2.5 < 10 -> `continue`, the pixels still counted
    r, = ref.centernet_localize([det], DEPTH, M)
    assert not r["valid"] and r["n_pixels"] == 2 and r["x"] == r["y"] == r["z"] == 0.0


def test_swapped_corners():
    a, = ref.centernet_localize([(0.25, 0.5, 0.25, 0.5)], DEPTH, M)
    for h, w in ((0.25, -0.5), (-0.25, 0.5), (-0.25, -0.5)):
        b, = ref.centernet_localize([(0.25, 0.5, h, w)], DEPTH, M)
        assert a == b


def test_all_zero_region_is_skipped():
    # e_x = 1.5, W = 3: columns 0 .. 2; e_y = 3, H = 1: rows int(2.6) = 2 .. int(3.4) = 3 -> all zero
    r, = ref.centernet_localize([(0.75, 0.25, 0.25, 0.5)], DEPTH, M)
    assert not r["valid"] and r["n_pixels"] == 0 and r["depth_sum"] == 0.0
    r, = ref.centernet_localize([(0.75, 0.25, 0.25, 0.5)], DEPTH, M, min_depth_sum=0, min_z=0)
    assert not r["valid"]


def test_non_finite_box_is_invalid():
    for det in ((0.5, 0.5, float("nan"), 0.5), (0.5, float("inf"), 0.5, 0.5)):
        r, = ref.centernet_localize([det], DEPTH, M)
        assert not r["valid"] and r["n_pixels"] == 0


def test_rectangle_fill():
    img = np.zeros((4, 6), dtype=np.uint8)
    ref.rectangle_fill(img, (4, 3), (-2, 2), 255)  # corners in the other order, clipped on the left
    want = np.zeros((4, 6), dtype=np.uint8)
    want[2:4, 0:5] = 255
    assert (img == want).all()
    img[:] = 0
    ref.rectangle_fill(img, (6, 0), (9, 3), 255)  # wholly outside
    assert not img.any()


def test_mask_mode_2x3():
    # nearest map of a 2 x 3 mask on 4 x 6: source column floor(xx / 2), source row floor(yy / 2)
    # > 0.5 at (0,0), (0,2), (1,1); 0.5 itself is not selected
    masks = torch.tensor([[[0.9, 0.5, 0.6], [0.1, 0.7, 0.5]]])
    box = torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.2, 0.2]])
    # (0,0): 1000 2000 1500 0; (0,2): 5000 6000 0 6500; (1,1): rows 2-3 x columns 2-3, all zero
    r, = ref.yolact_localize(masks, [1], box, DEPTH, 2.0, 4.0, 2.5, 2.0)
    assert r["valid"] and r["n_pixels"] == 6
    assert r["depth_sum"] == pytest.approx(22.0, rel=1e-14) and r["z"] == pytest.approx(22.0 / 6, rel=1e-14)
    assert r["e_x"] == 3.0 and r["e_y"] == 2.0
    assert r["x"] == pytest.approx(0.5 * (22.0 / 6 / 2), rel=1e-14) and r["y"] == 0.0
    # nothing above 0.5 -> the node's nanmean is NaN -> `continue`
    r, = ref.yolact_localize(torch.full((1, 2, 3), 0.5), [1], box, DEPTH, 2.0, 4.0, 2.5, 2.0)
    assert not r["valid"] and r["n_pixels"] == 0


def test_threshold_margin_helper():
    ok = [dict(n_pixels=5, depth_sum=19.0), dict(n_pixels=0, depth_sum=0.0)]
    ref.assert_clear_of_thresholds(ok, 10, 1)
    with pytest.raises(AssertionError):
        ref.assert_clear_of_thresholds([dict(n_pixels=5, depth_sum=10.0 + 1e-9)], 10, 1)
    with pytest.raises(AssertionError):
        ref.assert_clear_of_thresholds([dict(n_pixels=20, depth_sum=20.0)], 10, 1)


# ---- argument validation (before any launch; none of these touches a GPU) ----
def _det(y=0.5, x=0.5, h=0.2, w=0.2):
    return Detection(label=0, score=0.9, y=y, x=x, h=h, w=w)


def test_localize_detections_rejects_bad_arguments():
    with pytest.raises(ValueError, match="uint16"):
        loc.localize_detections([[_det()]], DEPTH.astype(np.float64), M)
    with pytest.raises(ValueError, match="uint16"):
        loc.localize_detections([[_det()]], torch.zeros(4, 6, dtype=torch.int16), M)
    with pytest.raises(ValueError, match="batch"):
        loc.localize_detections([[_det()], [_det()]], np.zeros((3, 4, 6), dtype=np.uint16), M)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        loc.localize_detections([[_det()]], np.zeros((6,), dtype=np.uint16), M)
    with pytest.raises(ValueError, match="M_projection"):
        loc.localize_detections([[_det()]], DEPTH, np.eye(2))
    with pytest.raises(ValueError, match="fx and fy"):
        loc.localize_detections([[_det()]], DEPTH, np.zeros((3, 3)))
    with pytest.raises(ValueError, match="per-image"):
        loc.localize_detections([_det()], DEPTH, M)


def test_localize_detections_without_detections_launches_nothing():
    assert loc.localize_detections([], DEPTH, M) == []
    assert loc.localize_detections([[], []], DEPTH, M) == [[], []]


def test_localize_masks_rejects_bad_arguments():
    masks, det, box = torch.zeros(2, 3, 2, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 5, 4)
    cam = (2.0, 4.0, 2.5, 2.0)
    with pytest.raises(ValueError, match="masks must be torch.float32"):
        loc.localize_masks(masks.double(), det, box, DEPTH, *cam)
    with pytest.raises(ValueError, match="det must be torch.int64"):
        loc.localize_masks(masks, det.int(), box, DEPTH, *cam)
    with pytest.raises(ValueError, match="batch mismatch"):
        loc.localize_masks(masks, det[:1], box, DEPTH, *cam)
    with pytest.raises(ValueError, match="batch mismatch"):
        loc.localize_masks(masks, det, box[:1], DEPTH, *cam)
    with pytest.raises(ValueError, match="counts"):
        loc.localize_masks(masks, det, box, DEPTH, *cam, counts=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="uint16"):
        loc.localize_masks(masks, det, box, DEPTH.astype(np.int32), *cam)
    with pytest.raises(ValueError, match="batch"):
        loc.localize_masks(masks, det, box, np.zeros((3, 4, 6), dtype=np.uint16), *cam)
    with pytest.raises(ValueError, match="fx and fy"):
        loc.localize_masks(masks, det, box, DEPTH, 0.0, 4.0, 2.5, 2.0)
    assert loc.localize_masks(masks[:, :0], det[:, :0], box, DEPTH, *cam).shape == (2, 0, 8)


def test_device_entry_points_reject_host_tensors_and_wrong_types():
    B, K = 2, 3
    rec, cnt = torch.zeros(B, K, 10), torch.zeros(B, dtype=torch.int32)
    depth = torch.zeros(B, 4, 6, dtype=torch.uint16)
    with pytest.raises(ValueError, match="records must be on the GPU"):
        loc.check_boxes_args(B, K, rec, cnt, depth, 1.0, 1.0)
    with pytest.raises(ValueError, match="records must be torch.float32"):
        loc.check_boxes_args(B, K, rec.half(), cnt, depth, 1.0, 1.0)
    with pytest.raises(ValueError, match="masks must be on the GPU"):
        loc.check_masks_args(B, K, torch.zeros(B, K, 2, 3), cnt, torch.zeros(B, K, dtype=torch.int64),
                             torch.zeros(B, 5, 4), depth, 1.0, 1.0)
    with pytest.raises(ValueError, match="GPU device"):
        loc.DeviceLocalizer(B, K, "cpu")
