"""Soft-NMS in the per-image merge (mbx_merge_detections_soft), the part that needs no GPU: the oracle of the GPU tests
(tests/soft_oracle.py) against answers known by hand and against the properties the definition promises -- among them the
gap condition that makes the exact-order comparison of the gaussian GPU tests legitimate --, the C-ABI table, and the
validation of DETECTION.MERGE_SOFT_NMS / MERGE_SOFT_NMS_SIGMA / MERGE_SOFT_NMS_MIN_SCORE."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_numpy as R
from multibox_amd.synth import merge_candidates
from tests import soft_oracle as S
from tests.merge_oracle import CASES
from tests.vote_oracle import iou_to as vote_iou_to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the hand-made three: IoU(A, B) = 4 / 8 exactly, C touches neither
KNOWN_BOXES = np.array([[[0, 0, 2, 2], [0, 0, 2, 4], [10, 10, 12, 12]]], np.float64)
KNOWN_SCORES = np.array([[0.75, 0.5, 0.25]], np.float32)
KNOWN_COUNT, KNOWN_ROWS = np.array([3], np.int32), np.array([0, 1], np.int32)


def known(method, thr=0.0, sigma=0.5, min_score=0.0, max_det=4):
    (k, t, gap, st), = S.soft_oracle(KNOWN_BOXES, KNOWN_SCORES, KNOWN_COUNT, KNOWN_ROWS, max_det, method, thr, sigma, min_score)
    return k.tolist(), t.tolist()


def test_known_answers():
    assert known(S.LINEAR, thr=0.3) == ([0, 1, 2], [0.75, 0.25, 0.25])   # B: 0.5 * (1 - 0.5), bit-equal with C: the lower index first
    assert known(S.LINEAR, thr=0.5) == ([0, 1, 2], [0.75, 0.5, 0.25])    # 0.5 is not > 0.5
    assert known(S.LINEAR, thr=0.3, min_score=0.3) == ([0], [0.75])      # B decays to 0.25 <= 0.3, C never was above it
    k, t = known(S.GAUSSIAN, sigma=0.5)
    assert k == [0, 1, 2] and t[0] == 0.75 and t[2] == 0.25
    assert t[1] == 0.5 * np.exp(-0.5) and abs(t[1] - 0.30326532985631671) < 1e-16
    assert known(S.LINEAR, thr=0.3, max_det=2)[0] == [0, 1]


def test_restated_iou_is_the_one_of_nms_greedy():
    b, s, c, ir = merge_candidates(seed=21, I=2, rows_per_image=(4, 7), K=40, n_obj=4)
    boxes = b.reshape(-1, 4)[:300]
    hits = 0
    for k0 in boxes[:5]:
        o = S.iou_to(k0, boxes)
        assert o.tobytes() == vote_iou_to(k0, boxes).tobytes()
        pair = np.array([R.nms_greedy(np.stack([k0, x]), 0.5).tolist() == [0] for x in boxes])      # x suppressed by k0 <=> IoU > .5
        assert np.array_equal(o > 0.5, pair) and not pair.all()
        hits += int(pair.sum())
    assert hits > 10
    assert S.weight(np.array([0.0, -0.0]), S.GAUSSIAN, 0, 0.5).tolist() == [1.0, 1.0]              # o == 0: exactly 1


@pytest.fixture(scope="module")
def case_inputs():
    return {name: merge_candidates(**kw) for name, (kw, _, _) in CASES.items()}


def top_n_of_the_live(scores, count, image_rows, max_det, min_score):
    """Per image: its candidates above min_score by score descending, ties by ascending flat index, cut to max_det."""
    out = []
    for i in range(len(image_rows) - 1):
        flat = S.image_candidates(scores, count, int(image_rows[i]), int(image_rows[i + 1]))
        s = scores.reshape(-1)[flat]
        flat, s = flat[s > np.float32(min_score)], s[s > np.float32(min_score)]
        out.append(flat[np.argsort(-s, kind="stable")][:max_det])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_properties_on_the_generator_cases(case_inputs, name):
    _, max_det, _ = CASES[name]
    b, s, c, ir = case_inputs[name]
    top = top_n_of_the_live(s, c, ir, max_det, 0.001)
    same = S.soft_oracle(b, s, c, ir, max_det, S.LINEAR, 1.0, 0.5, 0.001)                 # no IoU is > 1: nothing decays
    for (k, t, gap, st), want in zip(same, top):
        assert st == 0 and np.array_equal(k, want) and t.astype(np.float32).tobytes() == s.reshape(-1)[want].tobytes()
    for method, label in ((S.LINEAR, "linear 0.3"), (S.GAUSSIAN, "gaussian 0.5")):
        res = S.soft_oracle(b, s, c, ir, max_det, method, 0.3, 0.5, 0.001)
        print(name, label, "picks", [len(k) for k, _, _, _ in res], "smallest gap %.3g" % min(g for _, _, g, _ in res))
        for (k, t, gap, st), want in zip(res, top):
            assert st == 0 and len(k) > 0 and (np.diff(t) <= 0).all() and (t > 0.001).all()
            assert len(set(k.tolist())) == len(k)
            assert not np.array_equal(k, want) or t.astype(np.float32).tobytes() != s.reshape(-1)[want].tobytes()
            # the condition under which the device's pick ORDER may be compared with this one although its exp may differ
            # from numpy's in the last bit: wherever two live scores are not bit-equal they are 1e-9 apart, relative --
            # seven orders of magnitude above what a few hundred 1-ulp differences amount to
            if method == S.GAUSSIAN:
                assert gap > 1e-9, (name, gap)
    if name in ("typical", "wide"):
        assert all(len(k) == max_det for k, _, _, _ in res)
    if name == "small":                                                   # both exits of the loop are met: these stop short
        assert [len(k) for k, _, _, _ in S.soft_oracle(b, s, c, ir, max_det, S.LINEAR, 0.3, 0.5, 0.001)] == [16, 27, 12, 7, 56, 34]


def test_replay_reproduces_the_oracle_and_flags_a_wrong_order(case_inputs):
    b, s, c, ir = case_inputs["small"]
    flat = S.image_candidates(s, c, int(ir[4]), int(ir[5]))
    fb, fs = b.reshape(-1, 4)[flat], s.reshape(-1)[flat]
    picks, t, gap = S.soft_nms(fb, fs, 100, S.GAUSSIAN, 0.3, 0.5, 0.001)
    t_pick, t_best, was_live, left = S.replay(fb, fs, picks, S.GAUSSIAN, 0.3, 0.5, 0.001)
    assert t_pick.tobytes() == t.tobytes() and t_best.tobytes() == t.tobytes() and was_live.all() and left == -np.inf
    assert 1 < len(picks) < 100
    swapped = picks.copy()
    swapped[[0, -1]] = swapped[[-1, 0]]
    t_pick, t_best, was_live, left = S.replay(fb, fs, swapped, S.GAUSSIAN, 0.3, 0.5, 0.001)
    assert t_pick[0] < t_best[0]
    t_pick, t_best, was_live, left = S.replay(fb, fs, picks[:3], S.GAUSSIAN, 0.3, 0.5, 0.001)
    assert left == t[3]                                                   # stopped early: somebody is still live


def test_candidate_limit_and_timing_of_the_oracle():
    """640 picks among 16 384 candidates stay well under a second; one candidate more is status 1."""
    import time
    b, s, c, ir = merge_candidates(seed=12, I=1, rows_per_image=(82, 82), K=200, n_obj=30, count=200)
    c[81] = 184
    t0 = time.time()
    (k, t, gap, st), = S.soft_oracle(b, s, c, ir, 640, S.GAUSSIAN, 0.3, 0.5, 0.001)
    dt = time.time() - t0
    print("16 384 candidates, 640 picks: %.2f s" % dt)
    assert st == 0 and len(k) == 640
    c[81] = 185
    (k, t, gap, st), = S.soft_oracle(b, s, c, ir, 640, S.GAUSSIAN, 0.3, 0.5, 0.001)
    assert st == 1 and len(k) == 0
    ob, osc, src, cnt, stat = S.expected_arrays(b, [(k, t, gap, st)], 4)
    assert not ob.any() and not osc.any() and (src == -1).all() and cnt.tolist() == [0] and stat.tolist() == [1]


# ----------------------------------------------------------------------------------------------------------------- host side
def test_soft_entry_point_is_declared():
    from multibox_amd import _lib
    assert "mbx_merge_detections_soft" in _lib.declared_symbols()
    res, args = _lib._SIGS["mbx_merge_detections_soft"]
    assert len(args) == 19
    hdr = open(os.path.join(ROOT, "include", "mbx.h")).read()
    assert re.search(r"#define\s+MBX_SOFT_LINEAR\s+1\b", hdr) and re.search(r"#define\s+MBX_SOFT_GAUSSIAN\s+2\b", hdr)
    assert re.search(r"\bint\s+mbx_merge_detections_soft\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "NOT measured" in hdr[hdr.index("SOFT-NMS"):hdr.index("int mbx_merge_detections_soft")]       # the AP caveat


def test_soft_nms_validation():
    from multibox_amd import records as REC
    assert REC.merge_soft_nms(None, 0.5, 0.001) is None and REC.merge_soft_nms(None, "x", -1) is None
    assert REC.merge_soft_nms("linear", 0.5, 0.001) == (1, 0.5, 0.001) and REC.merge_soft_nms("gaussian", 1, 0) == (2, 1.0, 0.0)
    assert REC.merge_soft_nms("gaussian") == (2, 0.5, 0.001)
    for bad in ("Linear", "soft", "", 1, 2, True, False, 0.5, ["linear"]):
        with pytest.raises(ValueError, match="linear"):
            REC.merge_soft_nms(bad, 0.5, 0.001)
    for bad in (0, 0.0, -0.5, float("nan"), float("inf"), "nan", "x", None, True, [0.5]):
        with pytest.raises(ValueError, match="sigma"):
            REC.merge_soft_nms("gaussian", bad, 0.001)
    for bad in (-0.001, float("nan"), float("inf"), -float("inf"), "x", None, True, False, [0.1]):
        with pytest.raises(ValueError, match="minimum score"):
            REC.merge_soft_nms("linear", 0.5, bad)


def test_image_merger_argument_errors(monkeypatch):
    """ImageMerger checks soft= before it touches a GPU (the stream it opens is stubbed here)."""
    import torch
    from multibox_amd import detect as D
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: None)
    assert D.ImageMerger(50, 100, 0.5).soft is None and D.ImageMerger(50, 100, 0.5, soft=None).soft is None
    assert D.ImageMerger(50, 100, 0.5, soft=("linear", 0.5, 0.001)).soft == (1, 0.5, 0.001)
    assert D.ImageMerger(50, 100, None, soft=("gaussian", 0.25, 0.0), vote_iou=0.6).soft == (2, 0.25, 0.0)
    for iou in (None, float("nan")):
        with pytest.raises(ValueError, match="IoU threshold"):
            D.ImageMerger(50, 100, iou, soft=("linear", 0.5, 0.001))
    for bad in (("median", 0.5, 0.001), ("gaussian", 0.0, 0.001), ("gaussian", 0.5, -1.0), (True, 0.5, 0.001)):
        with pytest.raises(ValueError):
            D.ImageMerger(50, 100, 0.5, soft=bad)


@pytest.mark.parametrize("keys,named", [
    ("  MERGE_SOFT_NMS : median\n", "'linear', 'gaussian'"),
    ("  MERGE_SOFT_NMS : true\n", "'linear', 'gaussian'"),
    ("  MERGE_SOFT_NMS : gaussian\n  MERGE_SOFT_NMS_SIGMA : 0\n", "sigma"),
    ("  MERGE_SOFT_NMS : gaussian\n  MERGE_SOFT_NMS_SIGMA : .nan\n", "sigma"),
    ("  MERGE_SOFT_NMS : linear\n  MERGE_SOFT_NMS_MIN_SCORE : -0.5\n", "minimum score"),
    ("  MERGE_SOFT_NMS : linear\n  MERGE_IOU_THRESHOLD : null\n", "DETECTION.MERGE_IOU_THRESHOLD"),
])
def test_detect_cli_refuses_bad_soft_keys_before_the_gpu(tmp_path, keys, named):
    """detect.py stops at the config keys, before it selects a device or opens a checkpoint: this runs without a GPU."""
    cfg = tmp_path / "config.yaml"
    cfg.write_text("BATCH_SIZE : 4\nDETECTION :\n  USE_ORIGINAL_IMAGE : true\n" + keys)
    cmd = [sys.executable, os.path.join(ROOT, "detect.py"), "--priors", str(tmp_path / "none.pkl"), "--checkpoint_path",
           str(tmp_path), "--config", str(cfg), "--save_dir", str(tmp_path / "out"), "--synthetic", "4"]
    r = subprocess.run(cmd + ["--merge_per_image"], capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode != 0 and "MERGE_SOFT_NMS" in r.stderr and named in r.stderr, r.stderr[-2000:]
    assert "Traceback" not in r.stderr


def test_detect_cli_names_the_keys():
    src = open(os.path.join(ROOT, "detect.py")).read()
    for key in ("MERGE_SOFT_NMS", "MERGE_SOFT_NMS_SIGMA", "MERGE_SOFT_NMS_MIN_SCORE", "soft="):
        assert key in src
