"""tauv_vision_amd.augment on the host: the samplers (identity at p = 0, limits at p = 1, reproducible)
and the truth transforms on analytic cases. Nothing here touches a GPU."""
import math
from types import SimpleNamespace

import pytest
import torch

from tauv_vision_amd import augment as A

SRC, DST = (36, 50), (45, 70)


def _train_config(p, **over):
    """The reference's TrainConfig literals (yolact/scripts/train.py:51-81) with every *_p set to p."""
    c = dict(channel_shuffle_p=p, color_jitter_p=p, color_jitter_brightness=0.2, color_jitter_contrast=0.2,
             color_jitter_saturation=0.2, color_jitter_hue=0.2, gaussian_noise_p=p,
             gaussian_noise_var_limit=(10.0, 50.0), horizontal_flip_p=p, vertical_flip_p=p, blur_limit=(3, 7), blur_p=p,
             ssr_p=p, ssr_shift_limit=(-0.1, 0.1), ssr_scale_limit=(-0.1, 0.1), ssr_rotate_limit=(-30, 30),
             perspective_p=p, perspective_scale_limit=(0.0, 0.25), min_visibility=0.3)
    c.update(over)
    return SimpleNamespace(**c)


MODEL = SimpleNamespace(in_h=DST[0], in_w=DST[1])


def test_identity_params():
    p = A.identity_params(3, SRC, DST)
    assert p.records.shape == (3, A.REC) and p.records.dtype == torch.float32 and p.matrices.dtype == torch.float64
    want = torch.zeros(A.REC)
    want[[0, 4, 8]] = torch.tensor([SRC[1] / DST[1], SRC[0] / DST[0], 1.0])
    want[9:12] = torch.tensor([0.0, 1.0, 2.0])
    want[12:15] = 1
    want[A.BLUR_K] = 1
    assert torch.equal(p.records, want.expand(3, -1))
    assert torch.equal(p.matrices, A.resize_matrix(SRC, DST).expand(3, 3, 3))


def test_every_p_zero_is_the_identity():
    g = torch.Generator().manual_seed(1)
    p = A.sample_yolact_params(_train_config(0.0), MODEL, SRC, 5, g)
    ident = A.identity_params(5, SRC, DST)
    assert torch.equal(p.records, ident.records) and torch.equal(p.matrices, ident.matrices)
    assert p.min_visibility == 0.3
    g = torch.Generator().manual_seed(1)
    p = A.sample_centernet_params(SRC, DST, 5, g, crop_p=0, hsv_p=0, flip_p=0, blur_p=0, noise_p=0)
    assert torch.equal(p.records, ident.records) and torch.equal(p.matrices, ident.matrices)


def test_every_p_one_stays_inside_the_limits():
    g = torch.Generator().manual_seed(2)
    tc = _train_config(1.0)
    p = A.sample_yolact_params(tc, MODEL, SRC, 200, g)
    r = p.records.double()
    for slot in (A.BRIGHTNESS, A.CONTRAST, A.SATURATION):
        assert (r[:, slot] >= 0.8 - 1e-6).all() and (r[:, slot] <= 1.2 + 1e-6).all()
        assert r[:, slot].std() > 0.05
    assert (r[:, A.HUE].abs() <= 0.2 + 1e-6).all()
    var = r[:, A.NOISE_SIGMA] ** 2
    assert (var >= 10 - 1e-4).all() and (var <= 50 + 1e-4).all()
    assert set(r[:, A.BLUR_K].tolist()) == {3.0, 5.0, 7.0}
    assert (r[:, A.PERM:A.PERM + 3].sort(dim=1).values == torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)).all()
    assert len({tuple(x) for x in r[:, A.PERM:A.PERM + 3].tolist()}) > 1
    assert (r[:, 20:] == 0).all()
    # geometry: undo the known factors and look at what the ssr and perspective draws left
    S, Fl = A.resize_matrix(SRC, DST), A.flip_matrix(DST, True, True)  # p = 1: both flips
    for M in p.matrices:
        PR = M @ torch.linalg.inv(Fl @ S)
        # the projective row is the perspective's alone; its corner offsets lie in [0, 0.32)
        back = torch.linalg.inv(PR)
        corners = torch.tensor([[0, 0, 1], [DST[1], 0, 1], [DST[1], DST[0], 1], [0, DST[0], 1]], dtype=torch.float64)
        q = (back @ corners.T).T
        q = q[:, :2] / q[:, 2:]
        # R is a similarity about the centre with scale in [0.9, 1.1], |angle| <= 30, |shift| <= 0.1 of the
        # frame, and the perspective pulls each corner inward by < 0.32 of the frame: every pre-image of a
        # frame corner stays within this generous box
        assert (q[:, 0].abs() < 2.5 * DST[1]).all() and (q[:, 1].abs() < 2.5 * DST[0]).all()
        assert torch.isfinite(PR).all()
    g = torch.Generator().manual_seed(3)
    ssr_only = _train_config(0.0, ssr_p=1.0)
    for M in A.sample_yolact_params(ssr_only, MODEL, SRC, 200, g).matrices:
        Rm = M @ torch.linalg.inv(S)
        scale = math.hypot(float(Rm[0, 0]), float(Rm[0, 1]))
        angle = math.degrees(math.atan2(float(Rm[0, 1]), float(Rm[0, 0])))
        centre = Rm @ torch.tensor([DST[1] / 2, DST[0] / 2, 1.0], dtype=torch.float64)
        assert 0.9 - 1e-9 <= scale <= 1.1 + 1e-9 and abs(angle) <= 30 + 1e-9
        assert abs(float(centre[0]) - DST[1] / 2) <= 0.1 * DST[1] + 1e-9
        assert abs(float(centre[1]) - DST[0] / 2) <= 0.1 * DST[0] + 1e-9
        assert float(Rm[2, 0]) == 0 and float(Rm[2, 1]) == 0
    g = torch.Generator().manual_seed(4)
    for M in A.sample_yolact_params(_train_config(0.0, perspective_p=1.0), MODEL, SRC, 200, g).matrices:
        back = torch.linalg.inv(M @ torch.linalg.inv(S))
        corners = torch.tensor([[0, 0, 1], [DST[1], 0, 1], [DST[1], DST[0], 1], [0, DST[0], 1]], dtype=torch.float64)
        q = (back @ corners.T).T
        q = q[:, :2] / q[:, 2:] / torch.tensor([DST[1], DST[0]], dtype=torch.float64)
        inward = torch.stack([q[0], torch.stack([1 - q[1, 0], q[1, 1]]), 1 - q[2], torch.stack([q[3, 0], 1 - q[3, 1]])])
        assert (inward > -1e-9).all() and (inward < 0.32 + 1e-9).all()


def test_centernet_limits():
    g = torch.Generator().manual_seed(5)
    p = A.sample_centernet_params((360, 640), (360, 640), 200, g, crop_p=1, hsv_p=1, flip_p=1, blur_p=1, noise_p=1)
    r = p.records.double()
    assert (r[:, A.HUE].abs() <= 20 / 180 + 1e-6).all() and (r[:, A.SAT_SHIFT].abs() <= 30 / 255 + 1e-6).all()
    assert (r[:, A.VAL_SHIFT].abs() <= 20 / 255 + 1e-6).all()
    assert set(r[:, A.BLUR_K].tolist()) == {3.0, 5.0, 7.0}
    var = r[:, A.NOISE_SIGMA] ** 2
    assert (var >= 10 - 1e-4).all() and (var <= 50 + 1e-4).all()
    assert (r[:, A.BRIGHTNESS:A.SATURATION + 1] == 1).all()
    kinds = set()
    for M in p.matrices:
        kinds.add((float(M[0, 0]) < 0, float(M[1, 1]) < 0))
        # the crop window: height 260..360 rows of the 360, inside the frame
        back = torch.linalg.inv(M)
        c = (back @ torch.tensor([[0, 0, 1], [640, 360, 1]], dtype=torch.float64).T).T
        x, y = sorted(c[:, 0].tolist()), sorted(c[:, 1].tolist())
        assert 260 - 1e-6 <= y[1] - y[0] <= 360 + 1e-6 and -1e-6 <= y[0] and y[1] <= 360 + 1e-6
        assert -1e-6 <= x[0] and x[1] <= 640 + 1e-6
        assert abs((x[1] - x[0]) - min((y[1] - y[0]) * 640 / 360, 640)) < 1e-6
    assert kinds == {(True, False), (False, True), (True, True)}
    with pytest.raises(ValueError, match="unknown overrides"):
        A.sample_centernet_params((360, 640), (360, 640), 1, g, piecewise_affine_p=0.1)


def test_same_generator_state_same_records():
    a = A.sample_yolact_params(_train_config(0.5), MODEL, SRC, 16, torch.Generator().manual_seed(7))
    b = A.sample_yolact_params(_train_config(0.5), MODEL, SRC, 16, torch.Generator().manual_seed(7))
    c = A.sample_yolact_params(_train_config(0.5), MODEL, SRC, 16, torch.Generator().manual_seed(8))
    assert torch.equal(a.records, b.records) and torch.equal(a.matrices, b.matrices)
    assert not torch.equal(a.records, c.records)
    a = A.sample_centernet_params(SRC, DST, 16, torch.Generator().manual_seed(7))
    b = A.sample_centernet_params(SRC, DST, 16, torch.Generator().manual_seed(7))
    assert torch.equal(a.records, b.records) and torch.equal(a.matrices, b.matrices)


def test_records_invert_the_matrices():
    p = A.sample_yolact_params(_train_config(1.0), MODEL, SRC, 8, torch.Generator().manual_seed(9))
    minv = p.records[:, :9].double().view(8, 3, 3)
    prod = minv @ p.matrices
    prod = prod / prod[:, 2:, 2:]
    assert (prod - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-4
    # integer matrices invert exactly
    M = (A.flip_matrix((40, 40), True, False) @ A.shift_scale_rotate_matrix((40, 40), angle_deg=0.0))[None]
    assert torch.equal(A.params_from_matrices(M, (40, 40), (40, 40)).records[0, :9],
                       torch.tensor([-1.0, 0, 40, 0, 1, 0, 0, 0, 1]))


def test_params_refusals():
    eye = torch.eye(3, dtype=torch.float64)[None]
    with pytest.raises(ValueError, match="invertible"):
        A.params_from_matrices(torch.zeros(1, 3, 3), SRC, DST)
    with pytest.raises(ValueError, match="permutation"):
        A.params_from_matrices(eye, SRC, DST, perm=(0, 0, 2))
    with pytest.raises(ValueError, match="blur_k"):
        A.params_from_matrices(eye, SRC, DST, blur_k=4)
    with pytest.raises(ValueError, match="noise_sigma"):
        A.params_from_matrices(eye, SRC, DST, noise_sigma=-1.0)
    with pytest.raises(ValueError, match=r"\[B, 3, 3\]"):
        A.params_from_matrices(torch.eye(3), SRC, DST)


def _params(M, src=(40, 40), dst=(40, 40), mv=0.0):
    return A.params_from_matrices(M[None], src, dst, min_visibility=mv)


def test_boxes_hflip():
    box = torch.tensor([[[0.3, 0.2, 0.2, 0.1], [0.6, 0.9, 0.1, 0.2]]])
    valid = torch.tensor([[True, True]])
    out, v = A.transform_boxes(box, valid, _params(A.flip_matrix((40, 40), True, False)))
    want = box.clone()
    want[..., 1] = 1 - box[..., 1]
    assert v.all() and torch.allclose(out, want, atol=1e-6) and out.dtype == box.dtype
    pts, pv = A.transform_points(box[..., :2], valid, _params(A.flip_matrix((40, 40), True, False)))
    assert pv.all() and torch.allclose(pts, want[..., :2], atol=1e-6)


def test_boxes_quarter_turn_swaps_the_axes():
    # x' = y, y' = 40 - x: a quarter turn of the square frame about its centre
    M = torch.tensor([[0.0, 1, 0], [-1, 0, 40], [0, 0, 1]], dtype=torch.float64)
    box = torch.tensor([[[0.3, 0.2, 0.2, 0.1]]], dtype=torch.float64)
    out, v = A.transform_boxes(box, torch.tensor([[True]]), _params(M))
    assert v.all()
    assert torch.allclose(out, torch.tensor([[[1 - 0.2, 0.3, 0.1, 0.2]]], dtype=torch.float64), atol=1e-12)
    pts, pv = A.transform_points(box[..., :2], torch.tensor([[True]]), _params(M))
    assert pv.all() and torch.allclose(pts, torch.tensor([[[0.8, 0.3]]], dtype=torch.float64), atol=1e-12)


def test_box_pushed_outside_turns_invalid_in_place():
    M = torch.tensor([[1.0, 0, 60], [0, 1, 0], [0, 0, 1]], dtype=torch.float64)  # 60 px to the right of a 40 px frame
    box = torch.tensor([[[0.5, 0.5, 0.2, 0.2], [0.1, 0.1, 0.1, 0.1], [0.2, 0.8, 0.1, 0.1]]])
    valid = torch.tensor([[True, False, True]])
    out, v = A.transform_boxes(box, valid, _params(M))
    assert out.shape == box.shape and v.shape == valid.shape  # rows are not compacted
    assert not v.any() and (out == 0).all()
    pts, pv = A.transform_points(box[..., :2], valid, _params(M))
    assert pts.shape == (1, 3, 2) and not pv.any()
    # one row leaves, its neighbours keep their places
    M = torch.tensor([[1.0, 0, 20], [0, 1, 0], [0, 0, 1]], dtype=torch.float64)
    valid = torch.tensor([[True, True, True]])
    out, v = A.transform_boxes(box, valid, _params(M))
    assert v.tolist() == [[True, True, False]]
    assert torch.allclose(out[0, 1], torch.tensor([0.1, 0.6, 0.1, 0.1]), atol=1e-6)


def test_min_visibility_on_both_sides_of_a_half_clipped_box():
    # the box spans x in [0.4, 0.6]; shifted by 20 px of 40 it spans [0.9, 1.1]: exactly half is visible
    M = torch.tensor([[1.0, 0, 20], [0, 1, 0], [0, 0, 1]], dtype=torch.float64)
    box = torch.tensor([[[0.5, 0.5, 0.2, 0.2]]], dtype=torch.float64)
    valid = torch.tensor([[True]])
    out, v = A.transform_boxes(box, valid, _params(M), min_visibility=0.49)
    assert v.all() and torch.allclose(out, torch.tensor([[[0.5, 0.95, 0.2, 0.1]]], dtype=torch.float64), atol=1e-12)
    _, v = A.transform_boxes(box, valid, _params(M), min_visibility=0.51)
    assert not v.any()
    _, v = A.transform_boxes(box, valid, _params(M, mv=0.51))  # the params' own threshold is the default
    assert not v.any()


def test_truths_on_a_resize_keep_their_normalised_values():
    p = A.identity_params(2, SRC, DST)
    box = torch.tensor([[[0.5, 0.5, 0.2, 0.2]], [[0.25, 0.75, 0.1, 0.3]]])
    out, v = A.transform_boxes(box, torch.ones(2, 1, dtype=torch.bool), p)
    assert v.all() and torch.allclose(out, box, atol=1e-6)
