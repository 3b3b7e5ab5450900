"""The CenterNet loss tests' own tools, without a GPU: the shared input recipe (tests/centernet_loss_cases.py)
reproduces the stored fixtures' inputs bit for bit; its conditions on the inputs hold for every case,
stored or generated; and the tolerance rule of the GPU tests (centernet_loss_ref.check_values /
check_grads) reports each indexing defect the generated cases were made for when it is planted in the
fp32 restatement, and passes the restatement as it is."""
import numpy as np
import pytest
import torch

import centernet_loss_cases as C
import centernet_loss_ref as R
from helpers import golden
from oracle import ref_targets as rt

EVERY = list(C.CASES) + list(C.GENERATED)


@pytest.mark.parametrize("name", list(C.CASES))
def test_recipe_reproduces_the_stored_inputs(name):
    c = C.CASES[name]
    truth, _, view = C.make_inputs(c)
    made, g = C.stored_inputs(c, truth, view), golden(name)
    stored = [k for k in g.files if not k.startswith(("val_", "grad_"))]
    assert sorted(stored) == sorted(made)
    for k in stored:
        a = np.asarray(made[k])
        assert a.shape == g[k].shape and a.dtype == g[k].dtype, k
        np.testing.assert_array_equal(a, g[k], err_msg=k)  # NaN (the moduli of a label without angles) equal NaN
    # make_case and load_case hand the tests the same things
    _, mc, tc, oc, ltruth, lpred = R.load_case(name)
    mc2, tc2, oc2, truth2, pred2 = C.make_case(c)
    assert vars(mc2) == vars(mc) and vars(tc2) == vars(tc)
    assert (oc2.n_labels, oc2.n_keypoints) == (oc.n_labels, oc.n_keypoints)
    assert [[getattr(k, a).modulo for a in ("roll", "pitch", "yaw")] for k in oc2.configs] == \
        [[getattr(k, a).modulo for a in ("roll", "pitch", "yaw")] for k in oc.configs]
    for k in C.TRUTH:
        assert torch.equal(getattr(truth2, k), getattr(ltruth, k)), k
    for h in C.HEADS:
        assert (pred2[h] is None) == (lpred[h] is None) and (pred2[h] is None or torch.equal(pred2[h], lpred[h])), h


@pytest.mark.parametrize("name", EVERY)
def test_inputs_keep_off_the_discontinuities(name):
    c = C.spec_of(name)
    mc, tc, oc, truth, pred = C.make_case(c)
    for h in ("heatmap", "keypoint_heatmap"):
        if pred[h] is None:
            continue
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            z = pred[h].to(dt).float().abs().numpy()
            assert (np.abs(z - C.CLAMP_Z) >= C.LOGIT_BAND).all(), (h, dt)
        assert (pred[h].abs() >= 19.9).any()
    if c["moduli"] is not None:
        for axis, modulo in zip(("roll", "pitch", "yaw"), c["moduli"]):
            assert (C.angle_edge_distance(getattr(truth, axis), modulo, c["overlap"]) >= C.ANGLE_BAND).all(), axis
    for f in ("center", "keypoint_center"):
        p = getattr(truth, f)
        assert (C.cell_edge_distance(p, c) >= C.CELL_BAND).all(), f
        # so the fp32 cell (the reference's, the kernel's) is the float64 cell
        for k, n in enumerate((mc.in_h, mc.in_w)):
            assert torch.equal(((p[..., k] * n) / mc.downsample_ratio).to(torch.long),
                               ((p[..., k].double() * n) / mc.downsample_ratio).to(torch.long)), f


def test_generated_cases_hold_what_they_were_made_for():
    """The map sizes put each case on its schedule (256 threads a workgroup, four cells a thread on the
    vector route), and vec3's truth has the crowded cell and the shared corner cell."""
    cells = {n: (c["in_h"] >> c["ds"], c["in_w"] >> c["ds"]) for n, c in C.GENERATED.items()}
    assert cells == {"rows": (18, 30), "vec3": (36, 62), "scal3": (17, 31), "many": (4, 6)}
    for n, vector in (("rows", True), ("vec3", True), ("scal3", False), ("many", True)):
        assert ((cells[n][0] * cells[n][1]) % 4 == 0) == vector, n
    assert cells["rows"][1] % 4 == 2 and cells["vec3"][1] % 4 == 2  # a thread's four cells straddle rows
    assert C.GENERATED["many"]["B"] == 260 and C.GENERATED["scal3"]["focal"] == (2.5, 3.5)
    mc, tc, oc, truth, pred = C.make_case(C.GENERATED["vec3"])
    idx = rt.out_index_for_position(truth.center, mc)
    same = lambda b, objs: len({tuple(idx[b, o].tolist()) for o in objs}) == 1  # noqa: E731
    assert same(0, (0, 1)) and truth.valid[0, :3].all()
    assert same(1, (3, 4, 5, 6)) and truth.valid[1, 3:7].tolist() == [False, True, True, True]
    assert same(1, (7, 8)) and idx[1, 7].tolist() == [mc.out_h - 1, mc.out_w - 1] and truth.valid[1, 7:9].all()
    assert (truth.center[1, 7:9] > 1).all()
    others = [o for o in range(truth.valid.shape[1]) if o not in (3, 4, 5, 6)]
    assert not any(same(1, (3, o)) for o in others)  # object 3, invalid, is the first of its cell


# ---- the checks have teeth ------------------------------------------------------------------------

def _copy(name):
    v64, S, g64, v32, g32 = R.restated(name)
    return {t: float(v) for t, v in v32.items()}, {h: g.copy() for h, g in g32.items()}  # the cache stays as it is


def _focal_elements(name):
    """The fp32 restatement's focal elements (divided by N as focal_loss returns them) and positive counts
    of the heatmap and the keypoint heatmap, and the weighted affinity elements."""
    _, mc, tc, oc, truth, pred = R.case_inputs(name)
    a, b = tc.heatmap_focal_loss_a, tc.heatmap_focal_loss_b
    heat = rt.generate_heatmap(truth, mc, tc, oc.n_labels)
    kh, kw, ka = rt.generate_keypoint_heatmap(truth, mc, tc, oc.n_keypoints)
    eh, nh = R.focal_loss(torch.sigmoid(pred["heatmap"]), heat, a, b)
    ek, nk = R.focal_loss(torch.sigmoid(pred["keypoint_heatmap"]), kh, a, b)
    ea = kw.unsqueeze(2) * torch.nn.functional.mse_loss(pred["keypoint_affinity"], ka, reduction="none")
    positive = lambda t: torch.isclose(t, torch.ones(1))  # noqa: E731
    return tc, eh.double(), int(nh), ek.double(), int(nk), ea.double(), positive(kh)


def _values_reported(name, vals):
    v64, S, _, v32, _ = R.restated(name)
    with pytest.raises(AssertionError):
        R.check_values(vals, v64, S, v32)


def _grads_reported(name, grads):
    _, _, g64, _, g32 = R.restated(name)
    with pytest.raises(AssertionError):
        R.check_grads(grads, g64, g32)


@pytest.mark.parametrize("name", list(C.GENERATED))
def test_unmodified_restatement_passes(name):
    v64, S, g64, v32, g32 = R.restated(name)
    vals, grads = _copy(name)
    assert R.check_values(vals, v64, S, v32) <= 0.25 and R.check_grads(grads, g64, g32) <= 0.25
    for t in v32:
        assert np.isfinite(v32[t]) and np.isfinite(v64[t]), t


def test_dropped_partial_is_reported():
    """One dense workgroup of one plane (vec3 on the vector route: cells 1024..2047) left out of the sums."""
    tc, eh, nh, ek, nk, ea, _ = _focal_elements("vec3")
    assert nh > 0 and nk > 0
    vals, _ = _copy("vec3")
    vals["total"] = vals["heatmap"] = vals["total"] - float(eh[1, 0].reshape(-1)[1024:2048].sum())
    _values_reported("vec3", vals)
    vals, _ = _copy("vec3")
    drop_h = tc.loss_lambda_keypoint_heatmap * float(ek[0, 2].reshape(-1)[1024:2048].sum())
    drop_a = tc.loss_lambda_keypoint_affinity * float(ea[0, 2].reshape(2, -1)[:, 1024:2048].sum())
    vals["keypoint_heatmap"] -= drop_h
    vals["keypoint_affinity"] -= drop_a
    vals["total"] = vals["heatmap"] = vals["total"] - drop_h - drop_a
    _values_reported("vec3", vals)


def test_wrong_kind_is_reported():
    """finalize's split of the partials: one keypoint plane's sums and count taken for a heatmap plane's."""
    tc, eh, nh, ek, nk, ea, kpos = _focal_elements("vec3")
    plane, n_plane = float(ek[1, 0].sum()) * nk, int(kpos[1, 0].sum())  # the plane's sum before the division by N
    assert 0 < n_plane < nk
    vals, _ = _copy("vec3")
    heat = (float(eh.sum()) * nh + plane) / (nh + n_plane)
    kp = tc.loss_lambda_keypoint_heatmap * (float(ek.sum()) * nk - plane) / (nk - n_plane)
    vals["total"] = vals["heatmap"] = vals["total"] - float(eh.sum()) - vals["keypoint_heatmap"] + heat + kp
    vals["keypoint_heatmap"] = kp
    _values_reported("vec3", vals)


def test_wrong_row_is_reported():
    """rows: W = 30, so the vector of cells 28..31 holds the end of row 0 and the start of row 1; its four
    gradients written one row down."""
    W = C.GENERATED["rows"]["in_w"] >> C.GENERATED["rows"]["ds"]
    q = np.arange(28, 32)
    assert q[0] % 4 == 0 and q[0] // W != q[-1] // W
    for h in ("heatmap", "keypoint_heatmap"):
        _, grads = _copy("rows")
        flat = grads[h][1, 1].reshape(-1)  # a view of the copy
        moved = flat[q].copy()
        flat[q] = 0.0
        flat[q + W] = moved
        _grads_reported("rows", grads)


def test_dropped_sample_is_reported():
    """many: sample 256 (the first of the object kernel's last workgroup, finalize's second strided step)
    left out of the object sums: the object terms are those of the batch without it."""
    _, mc, tc, oc, truth, pred = R.case_inputs("many")
    assert truth.valid[256].any()
    keep = torch.arange(truth.valid.shape[0]) != 256
    rest = R.leaves({h: None if v is None else v[keep] for h, v in pred.items()}, torch.float32)
    short = R.loss_ref(rest, type(truth)(**{k: v[keep] for k, v in vars(truth).items()}), mc, tc, oc, torch.float32)[0]
    for t in ("size", "offset", "roll", "pitch", "yaw", "depth"):  # one term at a time, then all
        vals, _ = _copy("many")
        delta = float(short[t].detach()) - vals[t]
        assert delta != 0.0, t
        vals[t] += delta
        vals["total"] = vals["heatmap"] = vals["total"] + delta
        _values_reported("many", vals)
    vals, _ = _copy("many")
    for t in ("size", "offset", "roll", "pitch", "yaw", "depth"):
        delta = float(short[t].detach()) - vals[t]
        vals[t] += delta
        vals["total"] = vals["heatmap"] = vals["total"] + delta
    _values_reported("many", vals)


def test_ungathered_cell_is_reported():
    """vec3: the second object of a shared cell, and the last of the crowded one, not added to the cell's
    size gradient (lambda * valid * sign(prediction - truth) / n_valid, n_valid = 1)."""
    _, mc, tc, oc, truth, pred = R.case_inputs("vec3")
    idx = rt.out_index_for_position(truth.center, mc)
    for b, o in ((0, 1), (1, 6)):
        assert truth.valid[b, o]
        y, x = idx[b, o].tolist()
        _, grads = _copy("vec3")
        own = tc.loss_lambda_size * torch.sign(pred["size"][b, y, x] - truth.size[b, o]).double().numpy()
        assert np.abs(own).min() > 0
        grads["size"][b, y, x] -= own
        _grads_reported("vec3", grads)
