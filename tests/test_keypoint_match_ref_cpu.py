"""The replay checker of the keypoint matching (keypoint_match_ref.py) against the oracle's own
assignment: it accepts oracle.decode_keypoints on the planted scenes, rejects a swapped pair, a match
without a candidate and a stale slot_kp, the tie cap holds on the oracle side, and every scene has the
events the GPU tests rely on (contention for a slot, several candidates, no candidate)."""
import numpy as np
import pytest

import keypoint_match_ref as ref

CASES = [("A", 1), ("A", 2), ("A", 3), ("A", 5), ("A", 4), ("B", 1), ("B", 2), ("C", 1), ("C", 2), ("D", 1)]
# the events every case of a scene must contain (B cannot have a step without a candidate: see SCENES)
EVENTS = {"A": ("multi", "none", "excluded"), "B": ("multi", "excluded"), "C": ("multi", "none"),
          "D": ("multi", "none", "excluded")}
_CACHE = {}


def _case(name, seed):
    """(scene, records, oracle assignment, checker stats), computed once per case and never modified."""
    if (name, seed) not in _CACHE:
        scene = ref.make_scene(name, seed)
        rec = ref.oracle_records(scene)
        asg = ref.oracle_assignment(scene, rec)
        stats = ref.check_matching(*rec, scene.owner, scene.max_slots, *asg)
        _CACHE[(name, seed)] = (scene, rec, asg, stats)
    return _CACHE[(name, seed)]


@pytest.mark.parametrize("name,seed", CASES)
def test_checker_accepts_the_oracle_and_the_tie_cap_holds(name, seed):
    scene, (obj, obj_n, kp, kp_n), (kp_det, slot_kp, n_matched), stats = _case(name, seed)
    print(f"scene {name} seed {seed}: counts {obj_n.tolist()} / {kp_n.tolist()}, {stats}")
    assert stats["steps"] == int(kp_n.sum())
    for event in EVENTS[name]:
        assert stats[event] > 0, event
    ref.assert_tie_cap(stats, f"oracle, scene {name} seed {seed}")
    assert int((kp_det >= 0).sum()) == int(n_matched.sum()) == int((slot_kp >= 0).sum())


@pytest.mark.parametrize("seed", [1, 2, 3, 5])
def test_scene_a_seeds_without_a_tie(seed):
    """The seeds on which the GPU test also asserts equality with decode_keypoints."""
    assert _case("A", seed)[3]["tied"] == 0


def test_scene_shapes_take_both_table_routes():
    a, b = ref.SCENES["A"], ref.SCENES["B"]
    assert a["K"] * a["K_kp"] <= 4096 < b["K"] * b["K_kp"]
    assert max(b["slots"]) == 32 and b["K"] > 64 and 0 in a["slots"] and max(a["slots"]) == 8


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_checker_rejects_wrong_matchings(name):
    scene, rec, (kp_det, slot_kp, n_matched), _ = _case(name, 1)
    args = (*rec, scene.owner, scene.max_slots)
    # a swapped pair: the keypoint goes to another candidate, with slot_kp / n_matched consistent with that
    b, k, c, d2 = ref.multi_step(scene, rec, kp_det)
    bad = kp_det.copy()
    bad[b, k] = d2
    later = [j for j in range(scene.K_kp) if bad[b, j] == d2 and j != k
             and scene.owner[int(rec[2][b, j, 0])] == scene.owner[int(rec[2][b, k, 0])]]
    for j in later:  # the keypoint that held d2's slot takes c's: a swap
        bad[b, j] = c
    with pytest.raises(AssertionError, match="matched to|candidates"):
        ref.check_matching(*args, bad, *ref.assignment_arrays(bad, scene.K, scene.max_slots, scene.owner, rec[2]))
    # a match given where there is no candidate
    obj, obj_n, kp, kp_n = rec
    unmatched = [(b, k) for b in range(scene.B) for k in range(int(kp_n[b])) if kp_det[b, k] < 0]
    assert unmatched or name == "B"  # (every keypoint of scene B has a candidate)
    if unmatched:
        b, k = unmatched[0]
        bad = kp_det.copy()
        bad[b, k] = 0
        with pytest.raises(AssertionError, match="no candidate|candidates are"):
            ref.check_matching(*args, bad, *ref.assignment_arrays(bad, scene.K, scene.max_slots, scene.owner, kp))
    # a match at or past the count
    if kp_n[0] < scene.K_kp:
        bad = kp_det.copy()
        bad[0, kp_n[0]] = 0
        with pytest.raises(AssertionError, match="past the count"):
            ref.check_matching(*args, bad, slot_kp, n_matched)
    # a stale slot_kp row (a previous call's entry left behind), and a stale n_matched
    stale = slot_kp.copy()
    b, d, s = np.argwhere(stale < 0)[0]
    stale[b, d, s] = 0
    with pytest.raises(AssertionError, match="slot_kp"):
        ref.check_matching(*args, kp_det, stale, n_matched)
    stale = n_matched.copy()
    stale[0, scene.K - 1] += 1
    with pytest.raises(AssertionError, match="n_matched"):
        ref.check_matching(*args, kp_det, slot_kp, stale)


def test_checker_nan_affinity_goes_to_the_first_candidate():
    scene, rec, (kp_det, _, _), _ = _case("A", 1)
    obj, obj_n, kp, kp_n = (a.copy() for a in rec)
    b, k, c, _ = ref.multi_step(scene, rec, kp_det)
    kp[b, k, 8] = np.nan
    label, slot = scene.owner[int(kp[b, k, 0])]
    taken = {int(kp_det[b, j]) for j in range(k) if kp_det[b, j] >= 0 and scene.owner[int(kp[b, j, 0])] == (label, slot)}
    first = [d for d in range(int(obj_n[b])) if int(obj[b, d, 0]) == label and d not in taken][0]
    # replay the reference's loop with the NaN: every later step may change, so rebuild the assignment
    det = np.full_like(kp_det, -1)
    for bb in range(scene.B):
        used = set()
        for j in range(int(kp_n[bb])):
            from math import atan2
            lab, sl = scene.owner[int(kp[bb, j, 0])]
            cands = [d for d in range(int(obj_n[bb])) if int(obj[bb, d, 0]) == lab and (d, sl) not in used]
            if not cands:
                continue
            ang = atan2(float(kp[bb, j, 8]), float(kp[bb, j, 9]))
            errs = [abs(ang - atan2(float(kp[bb, j, 2]) - float(obj[bb, d, 2]), float(kp[bb, j, 3]) - float(obj[bb, d, 3])))
                    for d in cands]
            det[bb, j] = cands[errs.index(min(errs))]
            used.add((int(det[bb, j]), sl))
    assert det[b, k] == first
    stats = ref.check_matching(obj, obj_n, kp, kp_n, scene.owner, scene.max_slots, det,
                               *ref.assignment_arrays(det, scene.K, scene.max_slots, scene.owner, kp))
    assert stats["nan"] == 1
