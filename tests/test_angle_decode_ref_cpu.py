"""The yardstick of the orientation decode, on the CPU: angle_decode_ref.py's restatement against the
reference's own outputs (tests/golden/angles_b2_n64.npz, gen_golden_angles.py), the round trip through
angle_loss's encoding, the saturated-score rule, the period table, and the binding of the new entry.

The round-trip bound, reasoned (nothing here comes from the code under test): the decoded angle is an
fp32 value of up to 2 pi, where one ulp is 2^-21 = 4.8e-7. The fp32 sin / cos inputs move the angle by at
most 2^-24 * sqrt(2); atan2f is good to 2 ulp at pi (2 * 2^-22); the add of the bin centre, the remainder's
add and the scale's product round once each at up to 2 pi (3 * 2^-22); the scale constant is rounded once
(2^-24 * 2 pi). Together under 1.7e-6 < 4 * 2^-21 at period 2 pi, and in proportion for a shorter period."""
import os
import re
from math import pi

import numpy as np
import pytest
import torch

import angle_decode_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "angles_b2_n64.npz")
RANGES = {"two_pi": 2 * pi, "pi": pi, "half_pi": pi / 2}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_fixture_inputs_are_conditioned(golden):
    assert golden["bins"].shape == (2, 64, 4) and golden["offsets"].shape == (2, 64, 4)
    ref.assert_conditioned(golden["bins"])


@pytest.mark.parametrize("name", sorted(RANGES))
def test_fp32_restatement_is_bit_exact_to_the_reference(golden, name):
    got = ref.angle_decode_ref(golden["bins"], golden["offsets"], RANGES[name], torch.float32)
    assert got.dtype == np.float32 and np.array_equal(got, golden["angle_" + name])
    # the same with the period as a per-cell fp32 table, the form the device tests use
    per_cell = np.full((2, 64), RANGES[name], np.float32)
    assert np.array_equal(ref.angle_decode_ref(golden["bins"], golden["offsets"], per_cell, torch.float32), got)
    # and the package's own angle_decode (the parity API)
    from tauv_vision_amd.decode import angle_decode
    mine = angle_decode(torch.from_numpy(golden["bins"]), torch.from_numpy(golden["offsets"]), RANGES[name], pi / 3)
    assert np.array_equal(mine.numpy(), got)


@pytest.mark.parametrize("name", sorted(RANGES))
def test_float64_restatement_is_near_the_reference(golden, name):
    want = ref.angle_decode_ref(golden["bins"], golden["offsets"], RANGES[name], torch.float64)
    err = ref.circular_distance(golden["angle_" + name], want, RANGES[name]).max()
    print(f"reference fp32 vs float64 restatement at period {RANGES[name]:.4f}: {err:.3e}")
    assert err <= 4 * 2.0 ** -21 * RANGES[name] / (2 * pi)


@pytest.mark.parametrize("modulo", [2 * pi, pi / 2])
@pytest.mark.parametrize("overlap", [pi / 3, 0.0])
def test_round_trip_through_the_loss_encoding(modulo, overlap):
    theta = np.linspace(-7.0, 9.0, 96)  # either sign, more than one period, on no bin edge
    bins, offsets = ref.angle_encode(theta, modulo, overlap)
    assert bins.shape == (96, 4) and set(np.unique(bins)) == {-10.0, 10.0}
    for dtype, bound in ((torch.float32, 4 * 2.0 ** -21 * modulo / (2 * pi)), (torch.float64, 2.0 ** -23)):
        got = ref.angle_decode_ref(bins, offsets, modulo, dtype)
        assert ((got >= 0) & (got <= modulo * (1 + 2.0 ** -22))).all()  # (fp32(2 pi) lies above 2 pi)
        err = ref.circular_distance(got, theta % modulo, modulo).max()
        print(f"round trip, modulo {modulo:.4f}, overlap {overlap:.3f}, {dtype}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound  # (float64: only the fp32 rounding of the sin / cos inputs is left)


def test_saturated_scores_choose_bin_0():
    """(-15, 15) and (-20, 20) both give an fp32 score of exactly 1: `s1 > s0` is false and bin 0 is decoded.
    Comparing the logit differences (40 > 30) instead would decode bin 1 — in float64 the scores do differ."""
    bins = np.array([[-15.0, 15.0, -20.0, 20.0]], np.float32)
    s = torch.softmax(torch.from_numpy(bins).reshape(2, 2), dim=-1)[:, 1]
    assert s[0] == 1.0 and s[1] == 1.0
    offsets = np.array([[np.sin(0.3), np.cos(0.3), np.sin(1.1), np.cos(1.1)]], np.float32)
    got = ref.angle_decode_ref(bins, offsets, 2 * pi, torch.float32)
    assert abs(float(got[0]) - (pi / 2 + 0.3)) < 1e-6           # bin 0
    other = ref.angle_decode_ref(bins, offsets, 2 * pi, torch.float64)
    assert abs(float(other[0]) - (-pi / 2 + 1.1) % (2 * pi)) < 1e-6  # float64 would take bin 1


def test_angle_ranges():
    import tauv_vision_amd as tv
    A = tv.AngleConfig
    oc = tv.ObjectConfigSet([
        tv.ObjectConfig("square", A(True, pi / 2), A(False, pi), A(False, None), False, False, None),
        tv.ObjectConfig("free", A(True, 2 * pi), A(True, None), A(True, pi), False, False, None)])
    got = tv.angle_ranges(oc)
    assert got.dtype == np.float32 and got.shape == (3, 2)
    want = np.array([[np.nan, pi], [np.nan, np.nan], [pi / 2, 2 * pi]], np.float32)  # rows roll, pitch, yaw
    assert np.array_equal(got, want, equal_nan=True)
    # train=False with a modulo, and train=True without one: both "not decoded"
    assert np.isnan(got[1, 0]) and np.isnan(got[1, 1])


def test_records_to_detections_fills_the_angles():
    from tauv_vision_amd.decode import REC
    from tauv_vision_amd.sharding import records_to_detections
    rec = np.zeros((1, 3, REC), np.float32)
    rec[0, :, 1] = (0.9, 0.8, 0.7)
    ang = np.array([[[np.nan, 0.25, 1.5], [0.5, np.nan, np.nan], [9.0, 9.0, 9.0]]], np.float32)
    dets = records_to_detections(rec, np.array([2], np.int32), False, ang)
    assert [len(d) for d in dets] == [2]
    a, b = dets[0]
    assert (a.roll, a.pitch, a.yaw) == (None, 0.25, 1.5) and (b.roll, b.pitch, b.yaw) == (0.5, None, None)
    assert all(isinstance(v, float) for v in (a.pitch, a.yaw, b.roll))
    plain = records_to_detections(rec, np.array([2], np.int32), False)
    assert all(d.roll is None and d.pitch is None and d.yaw is None for d in plain[0])


def test_entry_is_declared_and_bound():
    from tauv_vision_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "tauv_vision_amd.h")).read()
    decl = re.search(r"int tv_decode_angles\(([^;]*)\);", text)
    assert decl and "tv_decode_angles" in _lib.EXPORTS
    assert len(decl.group(1).split(",")) == len(_lib.EXPORTS["tv_decode_angles"][0])
