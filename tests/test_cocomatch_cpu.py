"""Host side of the device COCO metric (multibox_amd/cocoeval.py: pack / match_host / accumulate, the path behind
eval.py --device_metric) against evaluate_bbox, which stays the oracle: the same twelve floats and lines, compared with ==.
No GPU: the matching comes from match_host (_evaluate_img) here; tests/test_gpu_cocomatch.py puts the kernel in its place."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from multibox_amd import cocoeval as CE
from multibox_amd.synth import coco_eval_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the inputs of tests/test_cocoeval_cpu.py
GT = [{"image_id": 1, "bbox": [10, 10, 50, 50], "area": 2500}, {"image_id": 1, "bbox": [100, 100, 40, 40], "area": 1600},
      {"image_id": 2, "bbox": [0, 0, 100, 100], "area": 10000}]
GT7 = [{"image_id": 7, "bbox": [0, 0, 100, 100], "area": 10000}]
HAND = {
    "perfect": (GT, [[1, 10, 10, 50, 50, 0.9, 1], [1, 100, 100, 40, 40, 0.8, 1], [2, 0, 0, 100, 100, 0.7, 1]]),
    "false_positive_between": (GT, [[1, 10, 10, 50, 50, 0.9, 1], [1, 200, 200, 40, 40, 0.8, 1], [2, 0, 0, 100, 100, 0.7, 1]]),
    "thresholds": (GT7, [[7, 10, 0, 100, 100, 0.5, 1]]),
    "duplicate_below": (GT7, [[7, 10, 0, 100, 100, 0.5, 1], [7, 10, 0, 100, 100, 0.4, 1]]),
    "worse_ranked_above": (GT7, [[7, 0, 0, 100, 100, 0.4, 1], [7, 30, 0, 100, 100, 0.9, 1]]),
    "no_detections": (GT, []),
    "no_gt": ([], [[1, 0, 0, 5, 5, 0.5, 1]]),
}
SEEDS = [11, 12, 13, 14, 15, 16]


def host_path(gt, dt):
    packed = CE.pack(gt, dt)
    return CE.accumulate(packed, *CE.match_host(packed))


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases_equal_evaluate_bbox(name):
    gt, dt = HAND[name]
    stats, lines = host_path(gt, dt)
    want_stats, want_lines = CE.evaluate_bbox(gt, dt)
    assert stats == want_stats and lines == want_lines


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sets_equal_evaluate_bbox(seed):
    """40 images, 0-13 gts, 0-130 detections (cut to 100), coordinates on a 0.5 px grid, eight score values."""
    gt, dt = coco_eval_set(seed, 40)
    stats, lines = host_path(gt, dt)
    want_stats, want_lines = CE.evaluate_bbox(gt, dt)
    print(seed, len(gt), len(dt), want_stats)
    assert stats == want_stats and lines == want_lines
    assert want_stats[0] > 0.0 and all(v > -1.0 for v in want_stats)                # every area range is met
    assert len(set(r[5] for r in dt)) == 8


def test_random_sets_have_ties_and_the_row_rule_agrees():
    """The sets hold equal IoUs within a detection's row and IoUs exactly on a threshold's side of interest, and
    _match_rows (the rule mbx_coco_match implements, naming the gt row) agrees with _evaluate_img wherever it matches."""
    gt, dt = coco_eval_set(SEEDS[0], 40)
    packed = CE.pack(gt, dt)
    matched, ignore, _ = CE.match_host(packed)
    tied = 0
    for i in range(len(packed.img_ids)):
        d, g = CE._image(packed, i)
        iou = CE._iou_xywh(d[:, :4], g[:, :4])
        tied += sum(len(np.unique(r[r >= 0.5])) < (r >= 0.5).sum() for r in iou)
        for ai, a_rng in enumerate(CE.AREA_RNG):
            rows = CE._match_rows(d, g, a_rng)
            assert np.array_equal(rows >= 0, matched[i, ai, :, :len(d)])
            in_rng = (g[:, 4] >= a_rng[0]) & (g[:, 4] <= a_rng[1])
            for ti in range(len(CE.IOU_THRS)):
                r = rows[ti][rows[ti] >= 0]
                assert len(set(r.tolist())) == len(r)                                # a gt is taken once
                assert np.array_equal(ignore[i, ai, ti, :len(d)][rows[ti] >= 0].astype(bool), ~in_rng[r])
    assert tied > 0


def test_pack_cuts_at_100_in_stable_order():
    dt = [[5, k, 0, 10, 10, [0.25, 0.5, 0.75][k % 3], 1] for k in range(130)]      # x = the input position
    dt += [[4, 0, 0, 10, 10, 0.5, 1]]
    packed = CE.pack([], dt)
    assert packed.img_ids == [4, 5] and packed.dt_rows.tolist() == [0, 1, 101] and packed.gt_rows.tolist() == [0, 0, 0]
    assert packed.dt_rows.dtype == packed.gt_rows.dtype == np.int32 and packed.dt.dtype == np.float64
    want = [k for k in range(130) if k % 3 == 2] + [k for k in range(130) if k % 3 == 1] + [k for k in range(130) if k % 3 == 0]
    assert packed.dt[1:, 0].tolist() == [float(k) for k in want[:100]]
    assert packed.dt[1:, 4].tolist() == [0.75] * 43 + [0.5] * 43 + [0.25] * 14
    # the float64 values are evaluate_bbox's: area falls back to w * h, ints become floats
    packed = CE.pack([{"image_id": 9, "bbox": [1, 2, 3, 4]}, {"image_id": 9, "bbox": [0.1, 0.2, 0.3, 0.7], "area": 5}], [])
    assert packed.gt.tolist() == [[1.0, 2.0, 3.0, 4.0, 12.0], [0.1, 0.2, 0.3, 0.7, 5.0]]


def test_images_with_only_gts_or_only_detections_are_kept():
    gt = [{"image_id": 3, "bbox": [0, 0, 50, 50], "area": 2500}, {"image_id": 1, "bbox": [0, 0, 40, 40], "area": 1600}]
    dt = [[2, 0, 0, 50, 50, 0.9, 1], [1, 0, 0, 40, 40, 0.8, 1]]
    packed = CE.pack(gt, dt)
    assert packed.img_ids == [1, 2, 3]
    assert np.diff(packed.dt_rows).tolist() == [1, 1, 0] and np.diff(packed.gt_rows).tolist() == [1, 0, 1]
    matched, ignore, n_gt = CE.match_host(packed)
    assert matched.shape == ignore.shape == (3, 4, 10, 100) and n_gt[:, 0].tolist() == [1, 0, 1]
    assert matched[0, 0, :, 0].all() and not matched[1].any() and not matched[2].any()
    stats, lines = CE.accumulate(packed, matched, ignore, n_gt)
    assert (stats, lines) == tuple(CE.evaluate_bbox(gt, dt))
    assert stats[0] > 0 and stats[8] == 0.5                                         # one of two gts found, one false positive


def test_coco_match_entry_point_is_declared():
    from multibox_amd import _lib, build as B
    res, args = _lib._SIGS["mbx_coco_match"]
    assert len(args) == 14
    hdr = open(os.path.join(ROOT, "include", "mbx.h")).read()
    assert re.search(r"#define\s+MBX_COCO_MAX_DET\s+100\b", hdr) and re.search(r"#define\s+MBX_COCO_MAX_GT\s+128\b", hdr)
    assert re.search(r"\bint\s+mbx_coco_match\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert CE.MAX_DET == 100 == CE.MAX_DETS[-1] and CE.MAX_GT == 128
    assert B.SOURCES["cocomatch.hip"] == ["-ffp-contract=off"]
    import __graft_entry__ as g
    g.build()
    assert hasattr(_lib.lib(), "mbx_coco_match")                                    # exported by the built library


def test_eval_cli_has_the_device_metric_flag():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--device_metric" in r.stdout
