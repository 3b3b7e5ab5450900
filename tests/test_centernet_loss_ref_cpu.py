"""The CenterNet loss without a GPU: the fp32 restatement (tests/centernet_loss_ref.py) reproduces the
reference's own values and gradients (tests/golden/loss_*.npz, made by gen_golden_loss.py from the
reference's loss() and total.backward()) bit for bit, so its float64 run is a sound yardstick for the
device; and the package's new names and entry points exist and agree across the header, capi.cpp and the
ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

import centernet_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", R.CASES)
def test_fp32_restatement_equals_reference_bit_for_bit(name):
    g, mc, tc, oc, truth, pred = R.load_case(name)
    p = R.leaves(pred, torch.float32)
    terms, S = R.loss_ref(p, truth, mc, tc, oc, torch.float32)
    terms["total"].backward()
    for t in R.TERMS:
        if "val_" + t in g.files:
            np.testing.assert_array_equal(terms[t].detach().numpy(), g["val_" + t], err_msg=t)
        else:
            assert t not in terms, t
    for h in R.HEADS:
        if pred[h] is not None:
            np.testing.assert_array_equal(getattr(p, h).grad.numpy(), g["grad_" + h], err_msg=h)
    assert S["total"] >= 0 or np.isnan(S["total"])


def test_fixtures_show_the_quirks():
    """The fixtures exercise what the docstring of loss() names: NaN without a valid object exactly in the
    terms divided by n_valid, a zero keypoint-heatmap term without a positive cell, gradients at invalid
    objects' cells through the angle terms."""
    g = R.load_case("loss_allheads_b2_24x40_novalid")[0]
    for t in ("total", "size", "offset", "roll", "pitch", "yaw", "depth", "avg_size_error"):
        assert np.isnan(g["val_" + t]), t
    for t in ("keypoint_heatmap", "keypoint_affinity", "max_size_error"):
        assert np.isfinite(g["val_" + t]), t
    assert np.isfinite(g["grad_heatmap"]).all() and np.isnan(g["grad_size"]).any()
    assert (g["grad_size"] == 0).any()  # cells no object was gathered from keep an exact zero
    e = R.load_case("loss_allheads_b2_24x40_nopositive")[0]
    assert float(e["val_keypoint_heatmap"]) == 0.0 and not e["grad_keypoint_heatmap"].any()
    g, mc, tc, oc, truth, pred = R.load_case("loss_allheads_b2_24x40")
    from oracle import ref_targets as rt
    idx = rt.out_index_for_position(truth.center, mc)
    b, o = [(b, o) for b in range(truth.valid.shape[0]) for o in range(truth.valid.shape[1]) if not truth.valid[b, o]][0]
    assert np.abs(g["grad_yaw_bin"][b, idx[b, o, 0], idx[b, o, 1]]).max() > 0


def test_fixture_logits_keep_off_the_clamp():
    ln = np.log(9999.0)
    for name in R.CASES[:3]:
        pred = R.load_case(name)[5]
        for h in ("heatmap", "keypoint_heatmap"):
            if pred[h] is None:
                continue
            for dt in (torch.float32, torch.float16, torch.bfloat16):
                z = pred[h].to(dt).float().abs().numpy()
                assert (np.abs(z - ln) >= 0.05).all(), (name, h, dt)
            assert (pred[h].abs() >= 19.9).any()


def test_new_names_import():
    from tauv_vision_amd import loss as L
    import tauv_vision_amd as tv
    assert tv.loss is L and callable(L.loss)  # the package attribute `loss` stays the module
    for n in ("Losses", "focal_loss", "angle_loss", "depth_loss", "angle_range", "angle_in_range", "Angle",
              "PoseSample"):
        assert getattr(tv, n) is getattr(L, n), n
    assert [f for f in L.Losses.__dataclass_fields__] == list(R.TERMS)
    for f in ("size", "roll", "pitch", "yaw", "depth"):
        assert f in L.PoseSample.__dataclass_fields__, f


def test_entry_points_agree():
    """The header declares, capi.cpp defines and _lib.py binds the same tv_centernet_loss_* functions with
    the same number of arguments, and the ctypes description has the header's size."""
    from tauv_vision_amd import _lib
    names = ["tv_centernet_loss_workspace_size", "tv_centernet_loss_dense", "tv_centernet_loss_objects",
             "tv_centernet_loss_finalize", "tv_centernet_loss_scale"]
    header = open(os.path.join(ROOT, "include", "tauv_vision_amd.h")).read()
    capi = open(os.path.join(ROOT, "tauv-vision_amd", "csrc", "capi.cpp")).read()
    for n in names:
        assert n in _lib.EXPORTS, n
        decl = re.search(r"\bint " + n + r"\(([^)]*)\);", header)
        defn = re.search(r"\bint " + n + r"\(([^)]*)\) \{", capi)
        assert decl and defn, n
        norm = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
        assert norm(decl.group(1)) == norm(defn.group(1)), n
        assert len(decl.group(1).split(",")) == len(_lib.EXPORTS[n][0]), n
    m = re.search(r"enum \{ TV_LOSS_HEATMAP = 0,([^}]*)\}", header)
    enum = ["heatmap"] + [s.strip()[len("TV_LOSS_"):].lower() for s in m.group(1).split(",")]
    assert enum == list(_lib.LOSS_TENSORS) + ["tensors"]
    # 9 int32 (+ 4 bytes padding), 10 + 6 doubles, 12 tensors of 2 pointers + 10 int64, 13 pointers
    assert __import__("ctypes").sizeof(_lib.LossDesc) == 40 + 16 * 8 + 12 * 96 + 13 * 8
