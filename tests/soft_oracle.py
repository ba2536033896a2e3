"""The oracle of the Soft-NMS tests (mbx_merge_detections_soft): the definition of include/mbx.h restated in numpy, one
vectorised step per pick -- never built from the code under test.  The IoU is oracle.ref_numpy.nms_greedy's, term by term
(tests/test_soft_cpu.py ties the two); every other operation is one rounded float64 operation in the order the header gives,
so the linear method is exact and the gaussian one is exact but for exp."""
import numpy as np

from oracle import ref_numpy as R  # noqa: F401  (the IoU restated below)
from tests.merge_oracle import CAND_LIMIT

LINEAR, GAUSSIAN = 1, 2


def iou_to(pick_box, cand_boxes):
    """IoU of the picked box p with every candidate c, float64, in R.nms_greedy's operation order with p as the EARLIER box."""
    e = np.asarray(pick_box, np.float64).reshape(4)
    b = np.asarray(cand_boxes, np.float64).reshape(-1, 4)
    ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.minimum(e[2], b[:, 2]) - np.maximum(e[0], b[:, 0])
    ih = np.minimum(e[3], b[:, 3]) - np.maximum(e[1], b[:, 1])
    inter = np.where((iw > 0.0) & (ih > 0.0), iw * ih, 0.0)
    union = (e[2] - e[0]) * (e[3] - e[1]) + ab - inter
    pos = union > 0.0
    return np.where(pos, inter / np.where(pos, union, 1.0), 0.0)


def weight(o, method, thr, sigma):
    if method == LINEAR:
        return np.where(o > np.float64(thr), 1.0 - o, 1.0)
    assert method == GAUSSIAN
    with np.errstate(all="ignore"):
        return np.exp(-((o * o) / np.float64(sigma)))


def is_live(t, min_score):
    with np.errstate(invalid="ignore"):
        return np.isfinite(t) & (t > np.float64(min_score))


def image_candidates(scores, count, r0, r1):
    """Flat indices (row * K + slot), ascending, of the candidates of rows [r0, r1): slots [0, clamp(count[r], 0, K))."""
    K = scores.shape[1]
    c = np.clip(np.asarray(count, np.int64), 0, K)
    return np.concatenate([np.arange(r * K, r * K + c[r]) for r in range(r0, r1)] + [np.zeros(0, np.int64)]).astype(np.int64)


def soft_nms(cand_boxes, cand_scores, max_det, method, thr, sigma, min_score):
    """Soft-NMS of one image's candidates, given in ascending flat-index order.  Returns (picks: positions in that order,
    t: the float64 working score of each pick when it was picked, gap: the smallest (best - runner-up) / best over the
    picks at which the two live scores are not bit-equal; inf when there is no such pick)."""
    b = np.asarray(cand_boxes, np.float64).reshape(-1, 4)
    t = np.asarray(cand_scores, np.float32).reshape(-1).astype(np.float64)
    live = is_live(t, min_score)
    picks, ts, gap = [], [], np.inf
    while len(picks) < max_det and live.any():
        tl = np.where(live, t, -np.inf)
        p = int(np.argmax(tl))                                            # the first of equal maxima: ascending flat index
        tl[p] = -np.inf
        r = tl.max()
        if r > -np.inf and r != t[p]:
            gap = min(gap, (t[p] - r) / t[p])
        picks.append(p)
        ts.append(t[p])
        live[p] = False
        with np.errstate(all="ignore"):
            t = np.where(live, t * weight(iou_to(b[p], b), method, thr, sigma), t)
        live &= is_live(t, min_score)
    return np.array(picks, np.int64), np.array(ts, np.float64), float(gap)


def replay(cand_boxes, cand_scores, picks, method, thr, sigma, min_score):
    """Every working score along a GIVEN pick sequence (positions in the candidates' order).  Returns (t_pick [n]: the pick's
    own working score when it was picked, t_best [n]: the largest live working score at that moment, was_live [n]: whether
    the pick was live then, t_left: the largest live working score after the last decay, -inf when nobody is live)."""
    b = np.asarray(cand_boxes, np.float64).reshape(-1, 4)
    t = np.asarray(cand_scores, np.float32).reshape(-1).astype(np.float64)
    live = is_live(t, min_score)
    t_pick, t_best, was_live = [], [], []
    for p in picks:
        p = int(p)
        t_pick.append(t[p])
        t_best.append(np.where(live, t, -np.inf).max() if len(t) else -np.inf)
        was_live.append(bool(live[p]))
        live[p] = False
        with np.errstate(all="ignore"):
            t = np.where(live, t * weight(iou_to(b[p], b), method, thr, sigma), t)
        live &= is_live(t, min_score)
    left = np.where(live, t, -np.inf).max() if len(t) else -np.inf
    return np.array(t_pick, np.float64), np.array(t_best, np.float64), np.array(was_live, bool), float(left)


def soft_oracle(boxes, scores, count, image_rows, max_det, method, thr, sigma, min_score, cand_limit=CAND_LIMIT):
    """Per image: (flat indices of the picks in pick order, their float64 working scores at pick time, the smallest gap,
    status).  An image above the candidate limit has status 1 and no picks."""
    fb, fs = np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(scores, np.float32).reshape(-1)
    out = []
    for i in range(len(image_rows) - 1):
        flat = image_candidates(scores, count, int(image_rows[i]), int(image_rows[i + 1]))
        if len(flat) > cand_limit:
            out.append((np.zeros(0, np.int64), np.zeros(0, np.float64), np.inf, 1))
            continue
        picks, t, gap = soft_nms(fb[flat], fs[flat], max_det, method, thr, sigma, min_score)
        out.append((flat[picks], t, gap, 0))
    return out


def expected_arrays(boxes, result, max_det):
    """The kernel's five outputs for soft_oracle's result: unused slots 0 / 0 / -1; scores are (float32)t."""
    n = len(result)
    ob, osc = np.zeros((n, max_det, 4), np.float64), np.zeros((n, max_det), np.float32)
    src, cnt, st = np.full((n, max_det), -1, np.int32), np.zeros((n,), np.int32), np.zeros((n,), np.int32)
    for i, (k, t, _, status) in enumerate(result):
        ob[i, :len(k)], osc[i, :len(k)] = np.asarray(boxes, np.float64).reshape(-1, 4)[k], t.astype(np.float32)
        src[i, :len(k)], cnt[i], st[i] = k, len(k), status
    return ob, osc, src, cnt, st
