"""Box voting in the per-image merge (mbx_merge_detections_voted), the part that needs no GPU: the oracle of the GPU tests
(tests/vote_oracle.py) against oracle.ref_numpy.nms_greedy and against answers known by hand, what voting is for, the
C-ABI table and the validation of DETECTION.MERGE_VOTE_IOU_THRESHOLD."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from oracle import ref_numpy as R
from multibox_amd.synth import merge_candidates
from tests.merge_oracle import candidate_order
from tests.vote_oracle import bound, image_candidates, iou_to, vote_exact, vote_members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_iou_rebuilds_nms_greedy():
    """The greedy keep list rebuilt from the vectorised IoU (> against the merge threshold) is R.nms_greedy's: the two are
    the same float64 expression, so voter membership (>= against the vote threshold) is exact as well."""
    b, s, c, ir = merge_candidates(seed=21, I=2, rows_per_image=(4, 7), K=40, n_obj=4)
    for i in range(2):
        boxes = b.reshape(-1, 4)[candidate_order(s, c, int(ir[i]), int(ir[i + 1]))]
        for thr in (0.3, 0.5):
            keep = []
            for j in range(len(boxes)):
                if not any(iou_to(boxes[k], boxes[j:j + 1])[0] > thr for k in keep):
                    keep.append(j)
            want = R.nms_greedy(boxes, thr)
            assert len(boxes) > 60 and 1 < len(want) < len(boxes) and keep == want.tolist()
        # one kept box against all candidates at once, as vote_members does it
        k0 = boxes[0]
        pair = np.array([R.nms_greedy(np.stack([k0, x]), 0.5).tolist() == [0] for x in boxes])      # x suppressed by k0 <=> IoU > .5
        assert np.array_equal(iou_to(k0, boxes) > 0.5, pair)


def test_known_answers_exact():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 12]], np.float64)
    scores = np.array([0.75, 0.25], np.float32)
    mean, absmean, n = vote_exact(boxes[:1], boxes, scores, 0.5)
    assert n.tolist() == [2] and mean[0] == [0, 0, 10, Fraction(21, 2)] and absmean[0] == mean[0]
    assert vote_members(boxes[0], boxes, scores, 0.5).tolist() == [True, True]
    # the >= rule: an IoU of exactly 0.5
    pair = np.array([[0, 0, 2, 2], [0, 0, 2, 4]], np.float64)
    assert iou_to(pair[0], pair).tolist() == [1.0, 0.5]
    assert vote_members(pair[0], pair, scores, 0.5).tolist() == [True, True]
    assert vote_members(pair[0], pair, scores, np.nextafter(0.5, 1)).tolist() == [True, False]
    mean, _, n = vote_exact(pair, pair, scores, 0.5)
    assert n.tolist() == [2, 2] and mean[0] == mean[1] == [0, 0, 2, Fraction(5, 2)]
    mean, _, n = vote_exact(pair, pair, scores, np.nextafter(0.5, 1))
    assert n.tolist() == [1, 1] and mean[0] == [0, 0, 2, 2] and mean[1] == [0, 0, 2, 4]


def test_non_voters_and_degenerate_boxes():
    boxes = np.tile([[0.0, 0.0, 10.0, 10.0]], (7, 1))
    scores = np.array([0.5, 0.0, -0.0, -1.0, np.nan, np.inf, 0.25], np.float32)
    assert vote_members(boxes[0], boxes, scores, 0.6).tolist() == [True, False, False, False, False, False, True]
    mean, absmean, n = vote_exact(boxes[:1], boxes, scores, 0.6)
    assert n.tolist() == [2] and mean[0] == [0, 0, 10, 10]
    flat = np.array([[1.0, 1.0, 1.0, 3.0]] * 2)                          # zero area: IoU 0 with everything, itself included
    mean, absmean, n = vote_exact(flat, flat, scores[:1].repeat(2), 0.6)
    assert n.tolist() == [0, 0] and mean == [None, None]
    assert bound(3, Fraction(1, 2)) == Fraction(10, 2 ** 53) * Fraction(1, 2)
    s = np.zeros((2, 3), np.float32)
    assert image_candidates(s, [2, 7], 0, 2).tolist() == [0, 1, 3, 4, 5] and image_candidates(s, [-1, 1], 0, 2).tolist() == [3]


@pytest.mark.parametrize("seed", range(100, 120))
def test_voting_localises_better_than_the_top_scoring_box(seed):
    """What the feature is for: 200 jittered copies of one true box; the voted box is closer to it than the copy the
    score happened to favour (the score says nothing about the jitter)."""
    rng = np.random.RandomState(seed)
    T = np.array([0.3, 0.25, 0.7, 0.8])
    cand = T + rng.normal(0, 0.01, (200, 4))
    scores = (np.floor(64 * rng.rand(200) + 1) / 64).astype(np.float32)
    top = int(np.argsort(-scores, kind="stable")[0])
    mean, _, n = vote_exact(cand[top:top + 1], cand, scores, 0.6)
    voted = np.array([float(v) for v in mean[0]])
    err_top, err_voted = np.abs(cand[top] - T).max(), np.abs(voted - T).max()
    print("seed", seed, "voters", int(n[0]), "error of the top-scoring box %.5f" % err_top, "of the voted box %.5f" % err_voted)
    assert n[0] > 100 and err_voted < 0.5 * err_top


def test_voted_entry_point_is_declared():
    from multibox_amd import _lib
    assert "mbx_merge_detections_voted" in _lib.declared_symbols()
    res, args = _lib._SIGS["mbx_merge_detections_voted"]
    assert len(args) == 16 and len(_lib._SIGS["mbx_merge_detections"][1]) == 14
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mbx_merge_detections_voted\s*\(", hdr) and re.search(r"\bint\s+mbx_merge_detections\s*\(", hdr)


def test_vote_threshold_validation():
    from multibox_amd import records as REC
    assert REC.merge_vote_iou(None) is None
    assert REC.merge_vote_iou(0.6) == 0.6 and REC.merge_vote_iou(1) == 1.0 and REC.merge_vote_iou(1e-3) == 1e-3
    for bad in (0, 0.0, -0.1, 1.5, "nan", float("nan"), float("inf"), "x", True, [0.5]):
        with pytest.raises(ValueError):
            REC.merge_vote_iou(bad)


def test_detect_cli_refuses_a_bad_vote_threshold_before_the_gpu(tmp_path, value="1.5"):
    """detect.py stops at the config key, before it selects a device or opens a checkpoint: this runs without a GPU."""
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE : 4\nDETECTION :\n  MERGE_IOU_THRESHOLD : 0.5\n  MERGE_VOTE_IOU_THRESHOLD : %s\n" % value)
    cmd = [sys.executable, os.path.join(ROOT, "detect.py"), "--priors", str(tmp_path / "none.pkl"), "--checkpoint_path",
           str(tmp_path), "--config", str(cfg), "--save_dir", str(tmp_path / "out"), "--synthetic", "4"]
    r = subprocess.run(cmd + ["--merge_per_image"], capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode != 0 and "DETECTION.MERGE_VOTE_IOU_THRESHOLD" in r.stderr and "(0, 1]" in r.stderr, r.stderr[-2000:]
    assert "Traceback" not in r.stderr


def test_detect_cli_names_the_key():
    src = open(os.path.join(ROOT, "detect.py")).read()
    assert "MERGE_VOTE_IOU_THRESHOLD" in src and "vote_iou=" in src
