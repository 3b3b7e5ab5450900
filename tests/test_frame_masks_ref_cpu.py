"""tests/frame_masks_ref.py against the fixture written from the reference's own assemble_mask, torch's
F.interpolate and numpy's float blend (tests/golden/gen_golden_frame_masks.py), bit for bit; TAB10
against matplotlib; the packed-bit layout's round trip. No GPU."""
import os

import numpy as np
import pytest
import torch

import frame_masks_ref as ref
from tauv_vision_amd.yolact import TAB10, pack_frame_masks, unpack_frame_masks

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_masks_k4_18x22_45x70.npz")
H, W = 45, 70


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
def test_restatement_equals_the_reference(golden, mode):
    mask = torch.from_numpy(golden["mask"]).unsqueeze(0)
    n = mask.shape[1]
    assert golden["frame"].shape == (H, W, 3) and int(golden["class_id"].max()) > 9
    sel = ref.selected(mask, [n], (H, W), mode)
    want = np.unpackbits(golden["sel_" + mode], axis=-1)[..., :W].astype(bool)
    assert np.array_equal(sel[0].numpy(), want)
    got = ref.blend(golden["frame"][None], sel, [n], golden["class_id"][None])
    assert got.dtype == np.uint8 and np.array_equal(got[0], golden["overlay_" + mode])
    # the order of the blend matters in this fixture (the detections overlap), and so does the count
    assert not np.array_equal(ref.blend(golden["frame"][None], sel.flip(1), [n], golden["class_id"][None, ::-1])[0],
                              golden["overlay_" + mode])
    assert not np.array_equal(ref.blend(golden["frame"][None], sel, [n - 1], golden["class_id"][None])[0],
                              golden["overlay_" + mode])


def test_the_two_modes_differ(golden):
    assert not np.array_equal(golden["sel_bilinear"], golden["sel_nearest"])


def test_rows_past_the_count_are_empty(golden):
    mask = torch.from_numpy(golden["mask"]).unsqueeze(0)
    sel = ref.selected(mask, [2], (H, W), "nearest")
    assert sel[0, :2].any() and not sel[0, 2:].any()


def test_tab10_is_the_references_colour():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps.get_cmap("tab10")
    for i in range(10):
        color = (255 * np.array(cmap(i))[:3])
        assert (int(color[0]), int(color[1]), int(color[2])) == tuple(int(v) for v in TAB10[i]), i
    assert cmap(12) == cmap(9)  # an index past the end takes the last colour
    assert np.array_equal(TAB10.numpy(), ref.TAB10)


def test_tab10_constant():
    assert TAB10.dtype == torch.uint8 and tuple(TAB10.shape) == (10, 3)
    assert np.array_equal(TAB10.numpy(), ref.TAB10)


@pytest.mark.parametrize("W_", [1, 31, 32, 33, 64, 65, 70, 127])
def test_pack_unpack_round_trip(W_):
    g = torch.Generator().manual_seed(W_)
    m = torch.rand((2, 3, 5, W_), generator=g) > 0.5
    m[0, 0, 0, :] = True   # every bit of a word set, the sign bit of its int32 view included
    m[1, 2, 4, :] = False
    bits = pack_frame_masks(m)
    assert bits.dtype == torch.uint32 and tuple(bits.shape) == (2, 3, 5, (W_ + 31) // 32)
    assert np.array_equal(bits.view(torch.int32).numpy().view(np.uint32), ref.pack(m.numpy()))
    assert torch.equal(unpack_frame_masks(bits, W_), m)
    assert torch.equal(unpack_frame_masks(bits.view(torch.int32), W_), m)
    # pixel x is bit x % 32 of word x // 32
    one = torch.zeros((1, W_), dtype=torch.bool)
    one[0, W_ - 1] = True
    word = pack_frame_masks(one).view(torch.int32).numpy().view(np.uint32)
    assert int(word[0, (W_ - 1) // 32]) == 1 << ((W_ - 1) % 32) and int(word.astype(np.uint64).sum()) == 1 << ((W_ - 1) % 32)


def test_unpack_refuses_a_wrong_width():
    bits = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError):
        unpack_frame_masks(bits, 97)
    with pytest.raises(ValueError):
        unpack_frame_masks(bits.float(), 70)
