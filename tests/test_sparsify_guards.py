"""CPU: neucon_network.sparsify_guards, the guards in front of a level's compaction (models/neucon_network.py:463-497), as a
table: the answer and the exact warning text at batch sizes 1 and 2, with the offending element first and last."""
import pytest

from eprecon_amd.config import EXCEED_NUM, STAGE_MIN_OCC
from eprecon_amd.neucon_network import sparsify_guards

CAP = 15000                              # cfg.TRAIN_NUM_SAMPLE[0]
OK = 9000                                # passes every guard
LOW = STAGE_MIN_OCC - 1
OVER = CAP + 1                           # over the cap, not over cap * EXCEED_NUM: sub-sampled
FAR = int(CAP * EXCEED_NUM) + 1
NO_POINTS = "no valid points: scale {}"
EXCEED = "exceed too many points: scale {} num_batch {}"
NO_TARGET = "occ_target is 0: scale {}"

# (scale, occupied, on_target, has_target, training) -> (subsample, warning)
TABLE = [
    # nothing to object to; the bounds themselves pass (the guards are strict inequalities)
    (0, [OK], [1], True, True, ([], None)),
    (1, [STAGE_MIN_OCC, CAP], [1, 1], True, True, ([], None)),
    # a count below STAGE_MIN_OCC, training or not
    (0, [LOW], [5], True, True, ([], NO_POINTS.format(0))),
    (2, [LOW], [5], True, False, ([], NO_POINTS.format(2))),
    (1, [LOW, OK], [5, 5], True, True, ([], NO_POINTS.format(1))),
    (1, [OK, LOW], [5, 5], True, True, ([], NO_POINTS.format(1))),
    (0, [0], [0], False, False, ([], NO_POINTS.format(0))),
    # training, a count above cap * EXCEED_NUM
    (0, [FAR], [5], True, True, ([], EXCEED.format(0, FAR))),
    (2, [FAR, OK], [5, 5], True, True, ([], EXCEED.format(2, FAR))),
    (2, [OK, FAR], [5, 5], True, True, ([], EXCEED.format(2, FAR))),
    # training, a count between cap and cap * EXCEED_NUM: sub-sample that element, no early return, target guard left open
    (0, [OVER], [5], True, True, ([0], None)),
    (0, [int(CAP * EXCEED_NUM)], [0], True, True, ([0], None)),
    (1, [OVER, OK], [5, 5], True, True, ([0], None)),
    (1, [OK, OVER], [5, 5], True, True, ([1], None)),
    (1, [OVER, OVER], [0, 5], True, True, ([0, 1], None)),
    # the reference's order: an element sub-sampled before a later one ends the forward, none after an earlier one did
    (1, [OVER, LOW], [5, 5], True, True, ([0], NO_POINTS.format(1))),
    (1, [LOW, OVER], [5, 5], True, True, ([], NO_POINTS.format(1))),
    (1, [OVER, FAR], [5, 5], True, True, ([0], EXCEED.format(1, FAR))),
    (1, [FAR, OVER], [5, 5], True, True, ([], EXCEED.format(1, FAR))),
    # the same counts outside training: the caps are ignored
    (0, [FAR], [5], True, False, ([], None)),
    (2, [FAR, OK], [5, 5], True, False, ([], None)),
    (2, [OK, FAR], [5, 5], True, False, ([], None)),
    (0, [OVER], [5], True, False, ([], None)),
    (1, [OVER, OK], [5, 5], True, False, ([], None)),
    (1, [OK, OVER], [5, 5], True, False, ([], None)),
    # no occupied voxel on an occupied target: ends the forward when there is a target, is not looked at when there is none
    (0, [OK], [0], True, True, ([], NO_TARGET.format(0))),
    (2, [OK], [0], True, False, ([], NO_TARGET.format(2))),
    (1, [OK, OK], [0, 5], True, True, ([], NO_TARGET.format(1))),
    (1, [OK, OK], [5, 0], True, True, ([], NO_TARGET.format(1))),
    (0, [OK], [0], False, True, ([], None)),
    (1, [OK, OK], [0, 5], False, False, ([], None)),
    (1, [OK, OK], [5, 0], False, True, ([], None)),
    # the count guards come first
    (0, [LOW], [0], True, True, ([], NO_POINTS.format(0))),
    (1, [OK, FAR], [0, 5], True, True, ([], EXCEED.format(1, FAR))),
]


@pytest.mark.parametrize("scale,occupied,on_target,has_target,training,want", TABLE)
def test_guard_table(scale, occupied, on_target, has_target, training, want):
    assert sparsify_guards(scale, occupied, on_target, has_target, training, CAP) == want


@pytest.mark.parametrize("on_target,has_target,want", [
    ([5], True, None), ([0], True, NO_TARGET.format(1)), ([0], False, None),
    ([0, 5], True, NO_TARGET.format(1)), ([5, 0], True, NO_TARGET.format(1)), ([5, 5], True, None), ([0, 0], False, None)])
def test_target_guard_after_the_sub_sampling(on_target, has_target, want):
    """sampled=True: the caller has cut the elements down as asked and counted again; the count guards were answered on the
    first call (here they would ask for the same sub-sampling again) and only the target guard is left"""
    occupied = [OVER] * len(on_target)
    assert sparsify_guards(1, occupied, on_target, has_target, True, CAP)[0] == list(range(len(on_target)))
    assert sparsify_guards(1, occupied, on_target, has_target, True, CAP, sampled=True) == ([], want)


def test_bounds_are_arguments():
    assert sparsify_guards(0, [40], [1], True, True, 30, exceed_num=2, min_occ=10) == ([0], None)
    assert sparsify_guards(0, [61], [1], True, True, 30, exceed_num=2, min_occ=10) == ([], EXCEED.format(0, 61))
    assert sparsify_guards(0, [9], [1], True, True, 30, exceed_num=2, min_occ=10) == ([], NO_POINTS.format(0))
