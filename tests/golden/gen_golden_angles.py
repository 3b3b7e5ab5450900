"""Golden fixture for the orientation decode (reference decode.py:291-316).

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER: it imports the reference's decode.py (through
gen_golden_targets._import_reference, whose stand-ins cover that file's imports), draws seeded bin logits
(under the condition of tests/angle_decode_ref.py) and offsets [2, 64, 4], runs the reference's
angle_decode in fp32 on the CPU for theta_range in {2 pi, pi, pi / 2} and stores inputs and outputs as
tests/golden/angles_b2_n64.npz. Data only: the reference source does not travel.
    python tests/golden/gen_golden_angles.py
"""
import os
import sys
from math import pi

import numpy as np
import torch

from gen_golden_targets import _import_reference

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from angle_decode_ref import assert_conditioned, conditioned_bins  # noqa: E402

RANGES = {"two_pi": 2 * pi, "pi": pi, "half_pi": pi / 2}


def main():
    _import_reference()
    from tauv_vision.centernet.model import decode as rdecode
    rng = np.random.default_rng(1705)
    bins = conditioned_bins(rng, (2, 64))
    assert_conditioned(bins)
    offsets = rng.normal(0.0, 1.0, (2, 64, 4)).astype(np.float32)
    out = {}
    for name, theta_range in RANGES.items():
        got = rdecode.angle_decode(torch.from_numpy(bins), torch.from_numpy(offsets), theta_range, pi / 3)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 64)
        out["angle_" + name] = got.numpy().copy()
        print(name, float(got.min()), float(got.max()))
    np.savez_compressed(os.path.join(HERE, "angles_b2_n64.npz"), bins=bins, offsets=offsets, **out)


if __name__ == "__main__":
    main()
