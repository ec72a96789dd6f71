"""CPU: the host half of the panoptic scoring (eprecon_amd/panoptic_score.py: finish, PanopticScore, the CLI's arguments)
against the issue's worked strip, hand-made tables for the greedy rule below 0.5, and the set-and-loop restatement of
tests/panoptic_score_ref.py.  Expected values are exact rationals; floats compare to 1e-12, integers exactly."""
import json

import numpy as np
import pytest

import panoptic_score_ref as R

TOL = 1e-12


@pytest.fixture(scope="module")
def PS():
    from eprecon_amd import panoptic_score
    return panoptic_score


def finish_of(PS, scene, threshold=0.5):
    return PS.finish(scene["M"], [k[0] for k in scene["pred_keys"]], [k[0] for k in scene["gt_keys"]], threshold)


assert_tables_equal = R.assert_tables_equal


def test_worked_strip(PS):
    pred, gt = R.strip()
    scene = R.score(pred, gt)
    assert scene["M"].shape == (5 + 1, 3 + 2) and scene["M"].sum() == 40
    assert scene["pred_keys"] == [(1, 0), (5, 7), (5, 8), (7, 9), (7, 10)] and scene["gt_keys"] == [(1, 0), (5, 3), (5, 4)]
    t = finish_of(PS, scene)
    assert_tables_equal(t, scene)
    at = {c: k for k, c in enumerate(t.classes)}
    assert [t.tp[at[1]], t.fp[at[1]], t.fn[at[1]]] == [1, 0, 0] and abs(t.iou_sum[at[1]] - 10 / 12) <= TOL
    assert [t.tp[at[5]], t.fp[at[5]], t.fn[at[5]]] == [1, 1, 1] and abs(t.iou_sum[at[5]] - 0.8) <= TOL
    assert [t.tp[at[7]], t.fp[at[7]], t.fn[at[7]]] == [0, 1, 0] and t.ignored == [3]          # instance 9: 5/5 on void
    s = PS.PanopticScore().add(t).summary()
    c1, c5, c7 = s["classes"]["1"], s["classes"]["5"], s["classes"]["7"]
    assert abs(c1["pq"] - 5 / 6) <= TOL and abs(c1["sq"] - 5 / 6) <= TOL and abs(c1["rq"] - 1.0) <= TOL
    assert abs(c5["pq"] - 0.4) <= TOL and abs(c5["sq"] - 0.8) <= TOL and abs(c5["rq"] - 0.5) <= TOL
    assert c7["pq"] == 0.0 and c7["sq"] == 0.0 and c7["rq"] == 0.0
    assert s["classes"]["3"]["pq"] is None and s["classes"]["3"]["iou"] is None
    assert s["all"]["n"] == 3 and abs(s["all"]["pq"] - (5 / 6 + 0.4 + 0.0) / 3) <= TOL
    assert s["stuff"]["n"] == 1 and abs(s["stuff"]["pq"] - 5 / 6) <= TOL
    assert s["things"]["n"] == 2 and abs(s["things"]["pq"] - 0.2) <= TOL
    # semantic: wall 10 / (10 + 2 + 0); chair 10 / (10 + 0 + 6): sites 10, 11 (wall on chair) and 20, 21, 24, 25 missed;
    # table: 4 sites on no ground truth, the 5 on void count nowhere
    assert abs(c1["iou"] - 10 / 12) <= TOL and abs(c5["iou"] - 10 / 16) <= TOL and c7["iou"] == 0.0
    assert [c7["sem_tp"], c7["sem_fp"], c7["sem_fn"]] == [0, 4, 0]
    assert abs(s["miou"] - (10 / 12 + 10 / 16 + 0.0) / 3) <= TOL
    R.assert_summaries_equal(s, R.summary([scene]))


def test_strip_at_a_quarter(PS):
    """the (5,4)/(5,8) pair has IoU 1/3: a match at 0.25, none at 0.5"""
    scene = R.score(*R.strip(), threshold=0.25)
    t = finish_of(PS, scene, 0.25)
    assert_tables_equal(t, scene)
    k = t.classes.index(5)
    assert [t.tp[k], t.fp[k], t.fn[k]] == [2, 0, 0] and abs(t.iou_sum[k] - (0.8 + 1 / 3)) <= TOL


def test_greedy_takes_the_larger_iou(PS):
    """one prediction p0 (20 sites) over two ground-truth chairs: 8 sites on g0 (12 sites), 10 on g1 (12 sites); IoU 8/24 and
    10/22, both candidates at 0.25: g1 wins, g0 is a false negative"""
    M = np.array([[8, 10, 0, 2],
                  [4, 2, 0, 0]], np.int64)
    t = PS.finish(M, [5], [5, 5], 0.25)
    assert [(p, g) for p, g, _ in t.matches] == [(0, 1)] and abs(t.matches[0][2] - 10 / 22) <= TOL
    k = t.classes.index(5)
    assert [t.tp[k], t.fp[k], t.fn[k]] == [1, 0, 1]
    want, taken, _ = R.match(M, [5], [5, 5], 0.25)
    assert want[5][:3] == [1, 0, 1] and [(p, g) for p, g, _ in taken] == [(0, 1)]
    # at 0.5 neither is a candidate
    t = PS.finish(M, [5], [5, 5], 0.5)
    assert [t.tp[k], t.fp[k], t.fn[k]] == [0, 1, 2]


def test_greedy_tie_goes_to_the_smaller_ground_truth_rank(PS):
    """p0 (18 sites) with 9 sites on each of g0 and g1 (12 sites each): IoU 9/21 twice; g0 is taken.  p1 (3 sites on g1) has
    IoU 3/12 = 0.25, not above the threshold: a false positive."""
    M = np.array([[9, 9, 0, 0],
                  [0, 3, 0, 0],
                  [3, 0, 0, 0]], np.int64)
    t = PS.finish(M, [5, 5], [5, 5], 0.25)
    assert [(p, g) for p, g, _ in t.matches] == [(0, 0)]
    k = t.classes.index(5)
    assert [t.tp[k], t.fp[k], t.fn[k]] == [1, 1, 1] and abs(t.iou_sum[k] - 9 / 21) <= TOL
    want, taken, _ = R.match(M, [5, 5], [5, 5], 0.25)
    assert want[5][:3] == [1, 1, 1] and [(p, g) for p, g, _ in taken] == [(0, 0)]
    # ... and two PREDICTIONS of 6 sites each inside one ground truth of 12 (IoU 1/2 twice): the smaller predicted rank
    M2 = np.array([[6, 0, 0],
                   [6, 0, 0],
                   [0, 0, 0]], np.int64)
    t = PS.finish(M2, [5, 5], [5], 0.25)
    assert [(p, g) for p, g, _ in t.matches] == [(0, 0)] and [t.tp[k], t.fp[k], t.fn[k]] == [1, 1, 0]
    assert [(p, g) for p, g, _ in R.match(M2, [5, 5], [5], 0.25)[1]] == [(0, 0)]


def test_classes_must_agree(PS):
    """a pair of different classes is no candidate whatever its overlap"""
    M = np.array([[10, 0, 0],
                  [0, 0, 0]], np.int64)
    t = PS.finish(M, [5], [6], 0.5)
    assert t.matches == [] and t.fp[t.classes.index(5)] == 1 and t.fn[t.classes.index(6)] == 1
    assert [t.sem_tp[t.classes.index(5)], t.sem_fp[t.classes.index(5)], t.sem_fn[t.classes.index(6)]] == [0, 10, 10]


def test_table_shape_is_checked(PS):
    with pytest.raises(ValueError):
        PS.finish(np.zeros((2, 3), np.int64), [5], [5, 5])


def random_scene(seed, n=400):
    """runs of 8 sites; the prediction is the ground truth with other instance ids, a fifth of the sites relabelled at random"""
    rng = np.random.default_rng(seed)
    sem, ins = np.repeat(rng.choice([0, 1, 2, 5, 5, 7, 40], n // 8), 8), np.repeat(rng.choice([1, 2, 3], n // 8), 8)
    gt = [None if rng.random() < 0.1 else g for g in R.gt_labels(sem, ins)]
    noise = rng.random(n) < 0.2
    p_sem = np.where(noise, rng.choice([0, 1, 5, 7, 9], n), np.where(sem == 40, 7, sem))      # (class indices 0..12 = their ids)
    pred = R.pred_labels(p_sem, np.where(noise, rng.choice([11, 12], n), ins + 10))
    return pred, gt


@pytest.mark.parametrize("threshold", [0.5, 0.25])
def test_two_scenes_pool(PS, threshold, tmp_path):
    scenes = [R.score(*random_scene(seed), threshold=threshold) for seed in (1, 2)]
    score = PS.PanopticScore()
    for scene in scenes:
        t = finish_of(PS, scene, threshold)
        assert_tables_equal(t, scene)
        score.add(t)
    want = R.summary(scenes, threshold)
    assert want["all"]["n"] >= 3 and sum(r["tp"] for r in want["classes"].values()) >= 2          # the scenes really score
    R.assert_summaries_equal(score.summary(), want)
    with open(score.write(str(tmp_path / "out" / "score.json"))) as fh:
        R.assert_summaries_equal(json.load(fh), want)
    text = PS.format_table(score.summary())
    assert text.splitlines()[0].split() == ["class", "PQ", "SQ", "RQ", "IoU", "TP", "FP", "FN"] and "mIoU" in text.splitlines()[-1]
    with pytest.raises(ValueError):
        score.add(finish_of(PS, scenes[0], 0.75))


def test_empty_score(PS):
    s = PS.PanopticScore().summary()
    assert s["scenes"] == 0 and s["all"] == {"n": 0, "pq": None, "sq": None, "rq": None} and s["miou"] is None


def test_cli_arguments(PS):
    a = PS.parse_args(["--pred", "p", "--scenes", "s.txt", "--gt", "g"])
    assert (a.pred, a.scenes, a.gt, a.info, a.threshold, a.out) == ("p", "s.txt", "g", None, 0.5, None)
    a = PS.parse_args(["--pred", "p", "--scenes", "s.txt", "--info", "i", "--threshold", "0.25", "--out", "o.json"])
    assert (a.gt, a.info, a.threshold, a.out) == (None, "i", 0.25, "o.json")
    for bad in (["--pred", "p", "--scenes", "s"], ["--pred", "p", "--scenes", "s", "--gt", "g", "--info", "i"],
                ["--scenes", "s", "--gt", "g"]):
        with pytest.raises(SystemExit):
            PS.parse_args(bad)


def test_cpu_tensors_are_refused(PS):
    import torch
    from eprecon_amd import _lib
    z = torch.zeros(4, dtype=torch.int32)
    for call in (lambda: PS.segment_table(z, z), lambda: PS.pair_counts(z, z, 1, 1), lambda: PS.score_sites(z, z, z, z)):
        with pytest.raises(_lib.EpreconError):
            call()
