"""The YOLACT loss without a GPU: the fp32 restatement (tests/yolact_loss_ref.py) reproduces the
reference's own values, gradients and sets (tests/golden/yolact_loss_*.npz, made by
gen_golden_yolact_loss.py from the reference's loss() and total.backward()) bit for bit, so its float64 run
is a sound yardstick for the device; make_inputs reproduces the stored inputs; every case meets the input
conditions of yolact_loss_cases.py; the new entry points agree across the header, capi.cpp and the ctypes
table; and the refusals fire before the library is reached."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import yolact_loss_cases as C
import yolact_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["tv_yolact_loss_workspace_size", "tv_yolact_loss_match", "tv_yolact_loss_select", "tv_yolact_loss_anchors",
           "tv_yolact_loss_mask_sums", "tv_yolact_loss_mask", "tv_yolact_loss_mask_coeff", "tv_yolact_loss_finalize"]


@pytest.mark.parametrize("name", R.CASES)
def test_fp32_restatement_equals_reference_bit_for_bit(name):
    g, c, cfg, inputs = R.load_case(name)
    pred = R.prediction_of(inputs, torch.float32)
    terms, S, st = R.loss_ref(pred, R.truth_of(inputs), cfg)
    terms["total"].backward()
    for t in R.TERMS:
        np.testing.assert_array_equal(terms[t].detach().numpy(), g["val_" + t], err_msg=t)
    for k, t in zip(C.PREDICTION, pred):
        if k in R.GRADS:
            got = t.grad if t.grad is not None else torch.zeros_like(t)
            np.testing.assert_array_equal(got.numpy(), g["grad_" + k], err_msg=k)
    pos = g["positive"].astype(bool)
    for k in ("positive", "negative", "selected"):
        np.testing.assert_array_equal(st[k].numpy(), g[k].astype(bool), err_msg=k)
    np.testing.assert_array_equal(st["match_index"].numpy()[pos], g["match_index"][pos])
    assert (g["match_index"][~pos] == -1).all()
    assert all(v >= 0 for v in S.values())


@pytest.mark.parametrize("name", R.CASES)
def test_make_inputs_reproduces_the_stored_inputs(name):
    g, c, cfg, inputs = R.load_case(name)
    assert int(g["seed"]) == c["seed"]
    made = C.make_inputs(c)
    assert sorted(made) == sorted(inputs)
    for k, v in made.items():
        assert v.dtype == inputs[k].dtype and torch.equal(v, inputs[k]), k


@pytest.mark.parametrize("name", R.CASES)
def test_input_conditions_hold(name):
    """On the stored inputs and on the generated ones, on the float64 restatement."""
    g, c, cfg, inputs = R.load_case(name)
    st = R.restated(name)[3]
    assert C.input_conditions(c, inputs, st) == []
    made = C.make_inputs(c)
    st = R.loss_ref(R.prediction_of(made, torch.float64), R.truth_of(made), cfg)[2]
    assert C.input_conditions(c, made, st) == []
    if c["invalid"] != "all":
        assert C.saturates(st)  # some mask logits pass both clamp bounds
        assert C.find_seed(c, first=c["seed"]) == c["seed"]


def test_input_conditions_report_what_they_are_for():
    """A threshold moved onto an anchor's IoU, a ratio past the negatives and a zero-height box are named."""
    name = "yolact_loss_a"
    g, c, cfg, inputs = R.load_case(name)
    st = dict(R.restated(name)[3])
    iou = float(st["match_iou"][st["positive"]].min())
    moved = dict(c)
    st_moved = dict(st, match_iou=st["match_iou"] - (iou - 0.5))
    assert any("pos threshold" in b for b in C.input_conditions(moved, inputs, st_moved))
    assert any("negatives" in b for b in C.input_conditions(dict(c, ratio=400), inputs, st))
    flat = {**inputs, "truth_box": inputs["truth_box"].clone()}
    flat["truth_box"][0, 0, 2] = 0.0
    assert any("height" in b for b in C.input_conditions(c, flat, st))


def test_fixtures_cover_what_the_cases_are_for():
    a, b, cc, d, e = (R.load_case(n)[0] for n in R.CASES)
    assert a["in_anchor"].shape[1] == 378 and 1100 <= b["in_anchor"].shape[1] <= 1600
    assert b["in_mask_prototype"].shape[1:] == (32, 23, 37) and cc["in_mask_coeff"].shape[2] == 5
    assert not a["in_truth_valid"].all() and not a["in_truth_img_valid"].all()
    for g in (a, b, cc, e):
        assert g["positive"].sum(axis=1).min() >= 1 and g["selected"].sum() == 4 * g["positive"].sum()
    # D: no positive, the three terms and every gradient exactly 0
    assert not d["positive"].any() and not d["selected"].any()
    assert all(float(d["val_" + t]) == 0.0 for t in R.TERMS)
    assert all(not d["grad_" + k].any() for k in R.GRADS)
    # E: the unpainted truths have positives, which the mask term skips: same classification and box
    # terms as A, a smaller mask term, and zero mask_coeff gradients at those positives
    c = C.CASES["yolact_loss_e"]
    for b_i, t in c["unpainted"]:
        assert not (e["in_truth_seg_map"][b_i] == t).any()
        rows = (e["match_index"][b_i] == t) & e["positive"][b_i].astype(bool)
        assert rows.any() and not e["grad_mask_coeff"][b_i][rows].any()
    assert float(e["val_box"]) == float(a["val_box"]) and float(e["val_mask"]) < float(a["val_mask"])
    for g in R.CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", g + ".npz")) < 953013


def test_entry_points_agree():
    """The header declares, capi.cpp defines and _lib.py binds the same tv_yolact_loss_* functions with the
    same arguments, and the ctypes description has the header's layout."""
    from tauv_vision_amd import _lib
    header = open(os.path.join(ROOT, "include", "tauv_vision_amd.h")).read()
    capi = open(os.path.join(ROOT, "tauv-vision_amd", "csrc", "capi.cpp")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    for n in ENTRIES:
        assert n in _lib.EXPORTS, n
        decl = re.search(r"\bint " + n + r"\(([^)]*)\);", header)
        defn = re.search(r"\bint " + n + r"\(([^)]*)\) \{", capi)
        assert decl and defn, n
        assert norm(decl.group(1)) == norm(defn.group(1)), n
        assert len(decl.group(1).split(",")) == len(_lib.EXPORTS[n][0]), n
    assert sorted(n for n in _lib.EXPORTS if n.startswith("tv_yolact_loss_")) == sorted(ENTRIES)
    body = re.search(r"typedef struct tv_yolact_loss_desc \{(.*?)\} tv_yolact_loss_desc;", header, re.S).group(1)
    names = []
    for stmt in body.split(";"):
        stmt = re.sub(r"\b(const|void|float|double|u?int\d+_t)\b", " ", stmt)
        names += [re.sub(r"\[.*", "", f).strip(" *\n") for f in stmt.split(",") if f.strip(" *\n")]
    assert names == [f[0] for f in _lib.YolactLossDesc._fields_]
    # 12 int32, 4 doubles, 18 pointers, 28 int64 strides
    assert ctypes.sizeof(_lib.YolactLossDesc) == 12 * 4 + 4 * 8 + 18 * 8 + 28 * 8


def test_new_names_import():
    from tauv_vision_amd import yolact_loss as L
    assert callable(L.loss) and callable(L.loss_with_state)
    assert "min(k, n_negative)" in L.loss.__doc__  # the departure is documented where the user reads it


def test_refusals_fire_before_the_library(monkeypatch):
    from tauv_vision_amd import _lib, yolact_loss as L

    def no_launch():
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_lib, "lib", no_launch)
    g, c, cfg, inputs = R.load_case("yolact_loss_a")

    def refused(match, cfg=cfg, **over):
        x = {**inputs, **over}
        with pytest.raises(ValueError, match=match):
            L.loss(tuple(x[k] for k in C.PREDICTION), tuple(x[k] for k in C.TRUTH), cfg)

    refused("on the host")
    refused("fp16 and bf16 are refused", mask_coeff=inputs["mask_coeff"].half())
    refused("fp16 and bf16 are refused", classification=inputs["classification"].bfloat16())
    refused("expected", box_encoding=inputs["box_encoding"][:, :-1])          # A
    refused("expected", mask_coeff=inputs["mask_coeff"][:1])                  # B
    refused("expected", mask_prototype=inputs["mask_prototype"][:, :-1])      # P
    refused("expected", anchor=inputs["anchor"][:, 1:])
    refused("T == 0", truth_valid=inputs["truth_valid"][:, :0], truth_classification=inputs["truth_classification"][:, :0],
            truth_box=inputs["truth_box"][:, :0])
    refused("negative_example_ratio", cfg=SimpleNamespace(**{**vars(cfg), "negative_example_ratio": -1}))
    refused("integers", truth_seg_map=inputs["truth_seg_map"].float())
