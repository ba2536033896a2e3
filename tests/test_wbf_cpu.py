"""Weighted boxes fusion without a GPU: the oracle of the GPU tests (tests/wbf_oracle.py) on hand-worked answers and
against the oracles it borrows from, the host-side argument checks (records.merge_wbf, ImageMerger(wbf=)) and detect.py's
DETECTION.MERGE_WBF keys as far as they are reached before a device is selected."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from multibox_amd.synth import merge_candidates
from oracle import ref_numpy as R
from tests import wbf_oracle as W
from tests.merge_oracle import CASES, merge_oracle
from tests.merge_oracle import expected_arrays as merge_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fuse(boxes, scores, conf=W.AVG, thr=0.55, min_score=0.0, views=1):
    """One image of one row: (fused boxes, scores, founders, members) as lists."""
    F, sc, first, n = W.wbf(np.array(boxes, np.float64), np.array(scores, np.float32), conf, thr, min_score, views)
    return F.tolist(), sc.tolist(), first.tolist(), n.tolist()


# ------------------------------------------------------------------------------------------------------- hand-worked answers
def test_iou_of_exactly_one_half_and_the_strict_rule():
    """[0,0,2,1] and [0,0,1,1]: inter 1, union 2 + 1 - 1 = 2, IoU 1/2 exactly."""
    boxes, scores = [[0, 0, 2, 1], [0, 0, 1, 1]], [0.75, 0.25]
    assert fuse(boxes, scores, thr=0.5) == ([[0, 0, 2, 1], [0, 0, 1, 1]], [0.75, 0.25], [0, 1], [1, 1])       # 0.5 is not > 0.5
    # just below: S = 0.75 + 0.25 = 1, X = 0.75 * [0,0,2,1] + 0.25 * [0,0,1,1] = [0,0,1.75,1], F = X / 1, score 1 / 2
    below = float(np.nextafter(0.5, 0.0))
    assert fuse(boxes, scores, thr=below) == ([[0, 0, 1.75, 1]], [0.5], [0], [2])
    assert fuse(boxes, scores, W.MAX, thr=below) == ([[0, 0, 1.75, 1]], [0.75], [0], [2])


def test_equal_overlap_joins_the_lower_cluster():
    """[1,0,3,2] between the clusters [0,0,2,2] and [2,0,4,2] (which touch, IoU 0): inter 2, union 4 + 4 - 2, IoU 1/3 with
    both.  It joins cluster 0: S = 0.75 + 0.25 = 1, X = 0.75 * [0,0,2,2] + 0.25 * [1,0,3,2] = [0.25, 0, 2.25, 2]; its score
    1 / 2 ties with cluster 1's 0.5 and the lower cluster number goes first."""
    boxes, scores = [[0, 0, 2, 2], [2, 0, 4, 2], [1, 0, 3, 2]], [0.75, 0.5, 0.25]
    assert fuse(boxes, scores, thr=0.3) == ([[0.25, 0, 2.25, 2], [2, 0, 4, 2]], [0.5, 0.5], [0, 1], [2, 1])
    assert fuse(boxes, scores, thr=0.34)[3] == [1, 1, 1]                  # 1/3 is not > 0.34
    # the same with the rows of the two clusters swapped: cluster 0 is now [2,0,4,2] (flat index 0 of equal scores)
    F, sc, first, n = fuse([[2, 0, 4, 2], [0, 0, 2, 2], [1, 0, 3, 2]], [0.5, 0.5, 0.25], thr=0.3)
    assert first == [1, 0] and n == [1, 2] and sc == [0.5, 0.375]         # (0.5 + 0.25) / 2
    assert F[1] == [(0.5 * 2 + 0.25 * 1) / 0.75, 0, (0.5 * 4 + 0.25 * 3) / 0.75, (0.5 * 2 + 0.25 * 2) / 0.75]


def test_candidates_are_matched_against_the_fused_box_not_the_first_member():
    """A = [0,0,4,4], B = [2,0,6,4], C = [3,0,7,4], all of area 16.  IoU(A, B) = 8 / 24 = 1/3 > 0.3: B joins A, the fused
    box of equal weights is [1,0,5,4].  IoU(fused, C) = 8 / 24 = 1/3: C joins.  IoU(A, C) = 4 / 28 = 1/7: matched against
    the first member alone C would have founded a second cluster."""
    boxes, scores = [[0, 0, 4, 4], [2, 0, 6, 4], [3, 0, 7, 4]], [0.5, 0.5, 0.25]
    assert W.iou_fused(np.array([[0., 0, 4, 4]]), np.array([16.]), np.array([3., 0, 7, 4]), 16.0)[0] == 4.0 / 28.0 < 0.3
    assert W.iou_fused(np.array([[1., 0, 5, 4]]), np.array([16.]), np.array([3., 0, 7, 4]), 16.0)[0] == 8.0 / 24.0 > 0.3
    # S = 1.25; X = [0.5 * 2 + 0.25 * 3, 0, 0.5 * 4 + 0.5 * 6 + 0.25 * 7, 1.25 * 4] = [1.75, 0, 6.75, 5]
    want = [1.75 / 1.25, 0.0, 6.75 / 1.25, 5.0 / 1.25]
    assert fuse(boxes, scores, thr=0.3) == ([want], [float(np.float32(1.25 / 3.0))], [0], [3])
    assert fuse(boxes[:2], scores[:2], thr=0.3)[0] == [[1, 0, 5, 4]]


@pytest.mark.parametrize("conf", [W.AVG, W.MAX])
def test_scores_and_expected_views(conf):
    """Clusters of 1, 2 and 6 identical boxes (disjoint from each other) under expected_views 1, 2 and 5: n below, equal to
    and above the number of views."""
    boxes = [[0, 0, 1, 1]] + [[2, 0, 3, 1]] * 2 + [[4, 0, 5, 1]] * 6
    scores = [0.5] + [0.75, 0.25] + [0.5, 0.25, 0.25, 0.25, 0.125, 0.125]
    q = {W.AVG: [0.5, 1.0 / 2.0, 1.5 / 6.0], W.MAX: [0.5, 0.75, 0.5]}[conf]     # clusters by founder: flat 0, 1, 3
    members = [1, 2, 6]
    for views in (1, 2, 5):
        F, sc, first, n = fuse(boxes, scores, conf, views=views)
        want = [float(np.float32(q[k] * min(members[k], views) / views)) if views > 1 else q[k] for k in range(3)]
        got = {f: (s, m) for f, s, m in zip(first, sc, n)}
        assert got == {0: (want[0], 1), 1: (want[1], 2), 3: (want[2], 6)}, views
        assert sc == sorted(sc, reverse=True)
    # five views: the lone box falls to a fifth, the pair to two fifths, the six stay
    assert fuse(boxes, scores, W.MAX, views=5)[1:3] == ([0.5, float(np.float32(0.75 * 2 / 5)), float(np.float32(0.5 / 5))], [3, 1, 0])


def test_who_takes_no_part():
    boxes = [[0, 0, 10, 10 + 0.25 * k] for k in range(9)]                 # all overlap heavily
    scores = [0.25, np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 0.5, 0.125]
    assert fuse(boxes, scores, thr=0.5)[2:] == ([7], [3])                 # 0.5, 0.25, 0.125
    assert fuse(boxes, scores, thr=0.5, min_score=0.125)[2:] == ([7], [2])      # at min_score: out
    assert fuse(boxes, scores, thr=0.5, min_score=float(np.nextafter(np.float32(0.125), np.float32(0))))[2:] == ([7], [3])
    assert fuse(boxes, [np.nan, np.inf, 0.0], thr=0.5) == ([], [], [], [])


# ---------------------------------------------------------------------------------------------------- against other oracles
def test_restated_iou_is_the_one_of_nms_greedy():
    b, s, c, ir = merge_candidates(seed=21, I=2, rows_per_image=(4, 7), K=40, n_obj=4)
    boxes = b.reshape(-1, 4)[:300]
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    hits = 0
    for k in (0, 17, 130):
        o = np.array([W.iou_fused(boxes[k:k + 1], areas[k:k + 1], x, a)[0] for x, a in zip(boxes, areas)])
        pair = np.array([R.nms_greedy(np.stack([boxes[k], x]), 0.5).tolist() == [0] for x in boxes])      # x suppressed by k <=> IoU > .5
        assert np.array_equal(o > 0.5, pair) and not pair.all()
        hits += int(pair.sum())
    assert hits > 10


def test_threshold_one_is_the_plain_top_n():
    kw, max_det, _ = CASES["topn"]
    b, s, c, ir = merge_candidates(**kw)
    s = s + np.float32(1 / 64)                                            # all live, ties kept
    eb, es, ei, ec = merge_expected(b, s, merge_oracle(b, s, c, ir, max_det, np.inf), max_det)
    for conf in (W.AVG, W.MAX):
        ob, osc, src, cnt, st, votes = W.expected_arrays(W.wbf_oracle(b, s, c, ir, conf, 1.0, 0.0, 1), max_det)
        assert ob.tobytes() == eb.tobytes() and osc.tobytes() == es.tobytes() and np.array_equal(src, ei) and np.array_equal(cnt, ec)
        assert not st.any() and np.array_equal(votes, (ei >= 0).astype(np.int32))


def test_the_seeded_cases_cross_any_resident_cluster_bound():
    """What the GPU tests lean on: `wide` has an image of more than 2 000 clusters, `clusters` one of more than 600 members."""
    for name, most_clusters, most_members in (("wide", 2035, 239), ("clusters", 33, 682)):
        b, s, c, ir = merge_candidates(**CASES[name][0])
        res = W.wbf_oracle(b, s, c, ir, W.AVG, 0.55, 0.0, 1)
        assert max(len(r[1]) for r in res) == most_clusters and max(int(r[3].max()) for r in res) == most_members
        for F, sc, first, n, status in res:
            assert status == 0 and (np.diff(sc) <= 0).all() and len(set(first.tolist())) == len(first)


def test_candidate_limit():
    b, s, c, ir = merge_candidates(seed=12, I=1, rows_per_image=(82, 82), K=200, n_obj=30, count=200)
    c[81] = 185                                                           # 81 * 200 + 185 = 16 385
    ob, osc, src, cnt, st, votes = W.expected_arrays(W.wbf_oracle(b, s, c, ir, W.AVG, 0.55, 0.0, 1), 10)
    assert not ob.any() and not osc.any() and (src == -1).all() and not votes.any() and cnt.tolist() == [0] and st.tolist() == [1]


# ----------------------------------------------------------------------------------------------------------------- host side
def test_wbf_entry_points_are_declared():
    from multibox_amd import _lib
    assert {"mbx_merge_detections_wbf", "mbx_merge_wbf_workspace"} <= set(_lib.declared_symbols())
    assert len(_lib._SIGS["mbx_merge_detections_wbf"][1]) == 21 and len(_lib._SIGS["mbx_merge_wbf_workspace"][1]) == 2
    hdr = open(os.path.join(ROOT, "include", "mbx.h")).read()
    assert re.search(r"#define\s+MBX_WBF_AVG\s+1\b", hdr) and re.search(r"#define\s+MBX_WBF_MAX\s+2\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mbx_merge_detections_wbf\s*\(", code) and re.search(r"\bsize_t\s+mbx_merge_wbf_workspace\s*\(", code)
    assert "NOT measured" in hdr[hdr.index("WEIGHTED BOXES FUSION"):hdr.index("int mbx_merge_detections_wbf")]      # the AP caveat


def test_merge_wbf_validation():
    from multibox_amd import records as REC
    assert REC.merge_wbf(None) is None and REC.merge_wbf(None, "x", -1, 0.5) is None
    assert REC.merge_wbf("avg") == (1, 0.55, 0.0, 1) and REC.merge_wbf("max", 0, 0.25, 2.0) == (2, 0.0, 0.25, 2)
    assert REC.merge_wbf("avg", 1, 0, 7) == (1, 1.0, 0.0, 7)
    for bad in ("Avg", "mean", "", 1, 2, True, False, 0.5, ["avg"]):
        with pytest.raises(ValueError, match="'avg', 'max'"):
            REC.merge_wbf(bad)
    for bad in (-0.001, 1.001, float("nan"), float("inf"), "0.5", "x", None, True, False, [0.5]):
        with pytest.raises(ValueError, match="IoU threshold"):
            REC.merge_wbf("avg", bad)
    for bad in (-0.001, float("nan"), float("inf"), -float("inf"), "0.1", None, True, False, [0.1]):
        with pytest.raises(ValueError, match="minimum score"):
            REC.merge_wbf("max", 0.55, bad)
    for bad in (0, -1, 1.5, float("nan"), float("inf"), 2.0 ** 31, "2", None, True, False, [2]):
        with pytest.raises(ValueError, match="expected views"):
            REC.merge_wbf("avg", 0.55, 0.0, bad)


def test_image_merger_argument_errors(monkeypatch):
    """ImageMerger checks wbf= before it touches a GPU (the stream it opens is stubbed here)."""
    import torch
    from multibox_amd import detect as D
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: None)
    assert D.ImageMerger(50, 100, 0.5).wbf is None and D.ImageMerger(50, 100, 0.5, wbf=None).wbf is None
    assert D.ImageMerger(50, 100, None, wbf=("avg", 0.55, 0.0, 2)).wbf == (1, 0.55, 0.0, 2)
    assert D.ImageMerger(50, 100, 0.5, wbf=("max",)).wbf == (2, 0.55, 0.0, 1)
    for kw in (dict(vote_iou=0.6), dict(soft=("gaussian", 0.5, 0.001)), dict(vote_iou=0.6, soft=("linear", 0.5, 0.001))):
        with pytest.raises(ValueError, match="vote_iou.*soft"):
            D.ImageMerger(50, 100, 0.5, wbf=("avg", 0.55, 0.0, 1), **kw)
    for bad in (("median", 0.55, 0.0, 1), ("avg", 1.5, 0.0, 1), ("avg", 0.55, -1.0, 1), ("avg", 0.55, 0.0, 0), (True, 0.55, 0.0, 1)):
        with pytest.raises(ValueError):
            D.ImageMerger(50, 100, 0.5, wbf=bad)


@pytest.mark.parametrize("keys,named", [
    ("  MERGE_WBF : mean\n", "'avg', 'max'"),
    ("  MERGE_WBF : avg\n  MERGE_WBF_IOU_THRESHOLD : 1.5\n", "IoU threshold"),
    ("  MERGE_WBF : max\n  MERGE_WBF_EXPECTED_VIEWS : 1.5\n", "expected views"),
    ("  MERGE_WBF_MIN_SCORE : 0.1\n", "MERGE_WBF_MIN_SCORE"),
    ("  MERGE_WBF : null\n  MERGE_WBF_EXPECTED_VIEWS : 2\n", "MERGE_WBF_EXPECTED_VIEWS"),
    ("  MERGE_WBF : avg\n  MERGE_SOFT_NMS : gaussian\n", "MERGE_SOFT_NMS"),
    ("  MERGE_WBF : avg\n  MERGE_VOTE_IOU_THRESHOLD : 0.6\n", "MERGE_VOTE_IOU_THRESHOLD"),
])
def test_detect_cli_refuses_bad_wbf_keys_before_the_gpu(tmp_path, keys, named):
    """detect.py stops at the config keys, before it selects a device or opens a checkpoint: this runs without a GPU."""
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE : 4\nDETECTION :\n  USE_ORIGINAL_IMAGE : true\n" + keys)
    cmd = [sys.executable, os.path.join(ROOT, "detect.py"), "--priors", str(tmp_path / "none.pkl"), "--checkpoint_path",
           str(tmp_path), "--config", str(cfg), "--save_dir", str(tmp_path / "out"), "--synthetic", "4"]
    r = subprocess.run(cmd + ["--merge_per_image"], capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode != 0 and "MERGE_WBF" in r.stderr and named in r.stderr, r.stderr[-2000:]
    assert "Traceback" not in r.stderr


def test_detect_cli_names_the_keys():
    src = open(os.path.join(ROOT, "detect.py")).read()
    for key in ("MERGE_WBF", "MERGE_WBF_IOU_THRESHOLD", "MERGE_WBF_MIN_SCORE", "MERGE_WBF_EXPECTED_VIEWS", "wbf="):
        assert key in src
