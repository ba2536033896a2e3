"""Result records of detect.py:438-460 as JSON text.  numpy + json only (no torch): detect.py runs these functions in
worker PROCESSES, off the thread that feeds the GPU."""
from __future__ import annotations

import json

import numpy as np


def results_to_json_text(boxes, scores, count, image_ids):
    """One string per record of detect.py:438-443 ({"image_id", "bbox", "score"} in patch order), byte for byte what
    json.dumps() writes for the record dicts (default separators, floats by the same C encoder) -- without building 70
    dicts per patch: "[" + ", ".join(all records) + "]" == json.dumps(list of dicts)."""
    boxes, scores, count = np.asarray(boxes), np.asarray(scores), np.asarray(count)
    out = []
    for b in range(boxes.shape[0]):
        n = int(count[b])
        if n == 0:
            continue
        head = '{"image_id": %s, "bbox": [' % json.dumps(image_ids[b])
        bb = json.dumps(boxes[b, :n].tolist())[2:-2].split("], [")        # '[[a, b, c, d], [..]]' -> ['a, b, c, d', ..]
        sc = json.dumps(scores[b, :n].tolist())[1:-1].split(", ")
        out.extend([head + x + '], "score": ' + s + "}" for x, s in zip(bb, sc)])
    return out


def batch_chunk(boxes, scores, count, image_ids):
    """(number of records, the records of one batch joined with ", ") -- one picklable string per batch."""
    recs = results_to_json_text(boxes, scores, count, image_ids)
    return len(recs), ", ".join(recs)


# ------------------------------------------------------------------ per-image merge (mbx_merge_detections): host side
MERGE_MAX_CANDIDATES = 16384           # MBX_MERGE_MAX_CANDIDATES (include/mbx.h)


def merge_vote_iou(value):
    """DETECTION.MERGE_VOTE_IOU_THRESHOLD / ImageMerger(vote_iou=): None = no box voting, else a float in (0, 1] (the
    range mbx_merge_detections_voted accepts); anything else is a ValueError."""
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (0.0 < v <= 1.0):
        raise ValueError("the vote IoU threshold must be a number in (0, 1] or null (no box voting), not %r" % (value,))
    return v


SOFT_NMS_METHODS = {"linear": 1, "gaussian": 2}      # MBX_SOFT_LINEAR, MBX_SOFT_GAUSSIAN (include/mbx.h)


def merge_soft_nms(method, sigma=0.5, min_score=0.001):
    """DETECTION.MERGE_SOFT_NMS, MERGE_SOFT_NMS_SIGMA and MERGE_SOFT_NMS_MIN_SCORE / ImageMerger(soft=): method None = no
    Soft-NMS (None is returned), else "linear" or "gaussian" and the validated (method id, sigma, min_score) that
    mbx_merge_detections_soft accepts: sigma a finite number > 0 (the width of the Gaussian weight exp(-IoU^2 / sigma); read
    by the gaussian method only, checked for both), min_score a finite number >= 0 (a candidate whose decayed score is at or
    below it is dropped).  Anything else, bools included, is a ValueError."""
    if method is None:
        return None
    if not isinstance(method, str) or method not in SOFT_NMS_METHODS:
        raise ValueError("the Soft-NMS method must be 'linear', 'gaussian' or null (no Soft-NMS), not %r" % (method,))

    def number(value):
        try:
            return float("nan") if isinstance(value, bool) else float(value)
        except (TypeError, ValueError):
            return float("nan")
    sg, ms = number(sigma), number(min_score)
    if not (0.0 < sg < float("inf")):
        raise ValueError("the Soft-NMS sigma (width of the Gaussian weight exp(-IoU^2 / sigma)) must be a finite number > 0, "
                         "not %r" % (sigma,))
    if not (0.0 <= ms < float("inf")):
        raise ValueError("the Soft-NMS minimum score (decayed scores at or below it are dropped) must be a finite number "
                         ">= 0, not %r" % (min_score,))
    return SOFT_NMS_METHODS[method], sg, ms


WBF_CONF_TYPES = {"avg": 1, "max": 2}                # MBX_WBF_AVG, MBX_WBF_MAX (include/mbx.h)


def merge_wbf(conf, iou_threshold=0.55, min_score=0.0, expected_views=1):
    """DETECTION.MERGE_WBF, MERGE_WBF_IOU_THRESHOLD, MERGE_WBF_MIN_SCORE and MERGE_WBF_EXPECTED_VIEWS / ImageMerger(wbf=):
    conf None = no weighted boxes fusion (None is returned), else "avg" or "max" (a cluster's score: the mean of its
    members' scores, or its first member's) and the validated (conf id, iou_threshold, min_score, expected_views) that
    mbx_merge_detections_wbf accepts: iou_threshold a number in [0, 1] (a candidate joins the cluster whose fused box it
    overlaps by more than this), min_score a finite number >= 0 (candidates at or below it take no part), expected_views
    an integer >= 1 (the number of patches that normally see an object; a cluster of fewer members is scaled down).
    Anything else, bools included, is a ValueError."""
    if conf is None:
        return None
    if not isinstance(conf, str) or conf not in WBF_CONF_TYPES:
        raise ValueError("the weighted boxes fusion score type must be 'avg', 'max' or null (no fusion), not %r" % (conf,))

    def number(value):
        try:
            return float("nan") if isinstance(value, (bool, str)) else float(value)
        except (TypeError, ValueError):
            return float("nan")
    thr, ms, ev = number(iou_threshold), number(min_score), number(expected_views)
    if not (0.0 <= thr <= 1.0):
        raise ValueError("the weighted boxes fusion IoU threshold (a candidate joins the cluster whose fused box it overlaps "
                         "by more than this) must be a number in [0, 1], not %r" % (iou_threshold,))
    if not (0.0 <= ms < float("inf")):
        raise ValueError("the weighted boxes fusion minimum score (candidates at or below it take no part) must be a finite "
                         "number >= 0, not %r" % (min_score,))
    if not (1.0 <= ev < 2.0 ** 31 and ev == int(ev)):
        raise ValueError("the weighted boxes fusion expected views (the number of patches that normally see an object) must "
                         "be an integer >= 1, not %r" % (expected_views,))
    return WBF_CONF_TYPES[conf], thr, ms, int(ev)


def group_rows(image_ids):
    """Runs of equal consecutive ids in stream order: (ids, image_rows [len(ids) + 1] int32); image i owns the rows
    [image_rows[i], image_rows[i + 1]).  An id that returns later is a new image; the padding rows of a partial batch
    carry the last image's id (and count 0), so they join it."""
    ids, starts = [], []
    for r, image_id in enumerate(image_ids):
        if not ids or image_id != ids[-1]:
            ids.append(image_id)
            starts.append(r)
    return ids, np.array(starts + [len(image_ids)], np.int32)


def score_order_keys(scores):
    """The order-preserving image of the float32 bits that the device sorts by (decode_filter_topk_kernel, merge_kernel):
    uint32, larger = earlier; -0 == +0, a NaN above everything."""
    s = np.ascontiguousarray(scores, np.float32)
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    key = np.where(s == 0, np.uint32(0x80000000), key)
    return np.where(np.isnan(s), np.uint32(0xffffffff), key).astype(np.uint32)


def best_candidates(scores, count, limit=MERGE_MAX_CANDIDATES):
    """Flat indices (row * K + slot, int64) of the best `limit` candidates of the rows scores [R,K] / count [R], in merge
    order: score descending, ties by ascending flat index."""
    scores, count = np.asarray(scores, np.float32), np.clip(np.asarray(count, np.int64), 0, scores.shape[1])
    flat = np.flatnonzero(np.arange(scores.shape[1])[None, :] < count[:, None])
    key = score_order_keys(scores.reshape(-1)[flat]).astype(np.int64)
    return flat[np.argsort(-key, kind="stable")][:limit]


def repack_rows(boxes, scores, flat, k_max):
    """The candidates `flat` (best_candidates) of boxes [R,K,4] / scores [R,K] as fresh rows of k_max slots, in that
    order -- what an image above the candidate limit is uploaded as.  Returns (boxes, scores, count)."""
    n = len(flat)
    rows = max(1, -(-n // k_max))
    b, s = np.zeros((rows * k_max, 4), np.float64), np.zeros((rows * k_max,), np.float32)
    b[:n], s[:n] = np.asarray(boxes).reshape(-1, 4)[flat], np.asarray(scores).reshape(-1)[flat]
    count = np.clip(n - np.arange(rows) * k_max, 0, k_max).astype(np.int32)
    return b.reshape(rows, k_max, 4), s.reshape(rows, k_max), count


def compact_rows(boxes, scores, count):
    """(count, valid boxes [n,4], valid scores [n]) of one batch: what a rank sends to rank 0 for the merge."""
    boxes, scores = np.asarray(boxes), np.asarray(scores)
    count = np.clip(np.asarray(count, np.int32), 0, scores.shape[1])
    valid = np.arange(scores.shape[1])[None, :] < count[:, None]
    return count.copy(), boxes[valid], scores[valid]


def expand_rows(count, boxes, scores, k_max):
    """Inverse of compact_rows: rows of k_max slots, unused slots zero."""
    count = np.asarray(count, np.int32)
    valid = np.arange(k_max)[None, :] < count[:, None]
    b, s = np.zeros((len(count), k_max, 4), np.float64), np.zeros((len(count), k_max), np.float32)
    b[valid], s[valid] = boxes, scores
    return b, s, count


def records_to_json(records):
    """The file detect.py:458-460 writes (json.dump of the record list) from record dicts, record strings or per-batch
    chunks of records (strings joined with ", "; empty chunks are skipped)."""
    if records and isinstance(records[0], str):
        return "[" + ", ".join(r for r in records if r) + "]"
    return json.dumps(records)
