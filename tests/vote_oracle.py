"""The oracle of the box-voting tests (mbx_merge_detections_voted), built from numpy, fractions and oracle.ref_numpy alone --
never from the code under test.  The IoU is oracle.ref_numpy.nms_greedy's, restated term by term and vectorised, so voter
membership is exact; the voted box is the exact rational sum(w x) / sum(w) of the float64 / float32 inputs."""
from fractions import Fraction

import numpy as np

from oracle import ref_numpy as R  # noqa: F401  (the definition restated below; tests/test_vote_cpu.py ties the two)


def iou_to(kept_box, cand_boxes):
    """IoU of one kept box e with every candidate b, float64, in R.nms_greedy's operation order: e is the EARLIER box
    (b[j] there), the candidate's area is the separate term `ai`, union > 0 ? inter / union : 0."""
    e = np.asarray(kept_box, np.float64).reshape(4)
    b = np.asarray(cand_boxes, np.float64).reshape(-1, 4)
    ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.minimum(e[2], b[:, 2]) - np.maximum(e[0], b[:, 0])
    ih = np.minimum(e[3], b[:, 3]) - np.maximum(e[1], b[:, 1])
    inter = np.where((iw > 0.0) & (ih > 0.0), iw * ih, 0.0)
    union = (e[2] - e[0]) * (e[3] - e[1]) + ab - inter
    pos = union > 0.0
    return np.where(pos, inter / np.where(pos, union, 1.0), 0.0)


def votable(cand_scores):
    """A candidate may vote iff its score is finite and > 0 (NaN, +-0, negatives and +inf do not)."""
    s = np.asarray(cand_scores, np.float32).reshape(-1)
    return np.isfinite(s) & (s > 0)


def vote_members(kept_box, cand_boxes, cand_scores, thr):
    """Boolean mask over the candidates: which of them vote for kept_box at vote IoU threshold thr (>=)."""
    return votable(cand_scores) & (iou_to(kept_box, cand_boxes) >= np.float64(thr))


def _dyadic(a):
    """float array -> (Python-int object array m, int64 array e) with a == m * 2**e exactly."""
    m, e = np.frexp(np.asarray(a, np.float64))
    return (m * 2.0 ** 53).astype(np.int64).astype(object), e.astype(np.int64) - 53


def _exact_sum(m, e):
    """sum(m * 2**e) as a Fraction; m Python ints (object array), e int64."""
    if len(m) == 0:
        return Fraction(0)
    e0 = int(e.min())
    total = int(np.sum(m * (2 ** (e - e0).astype(object))))
    return Fraction(total) * Fraction(2) ** e0


def vote_exact(kept_boxes, cand_boxes, cand_scores, thr):
    """Per kept box k and coordinate j: (mean[k][j], absmean[k][j], n[k]) with mean = sum(w x) / sum(w) and
    absmean = sum(w |x|) / sum(w) as exact Fractions over the voters of k (w the float32 score, x the float64
    coordinate), n the number of voters; mean[k] and absmean[k] are None where n[k] == 0."""
    kept = np.asarray(kept_boxes, np.float64).reshape(-1, 4)
    b = np.asarray(cand_boxes, np.float64).reshape(-1, 4)
    s = np.asarray(cand_scores, np.float32).reshape(-1)
    ok = votable(s)
    mw, ew = _dyadic(np.where(ok, s, 0).astype(np.float64))
    mx, ex = _dyadic(b)
    mean, absmean, n = [], [], np.zeros(len(kept), np.int64)
    for k in range(len(kept)):
        v = np.nonzero(ok & (iou_to(kept[k], b) >= np.float64(thr)))[0]
        n[k] = len(v)
        if len(v) == 0:
            mean.append(None)
            absmean.append(None)
            continue
        sw = _exact_sum(mw[v], ew[v])
        mean.append([_exact_sum(mw[v] * mx[v, j], ew[v] + ex[v, j]) / sw for j in range(4)])
        absmean.append([_exact_sum(mw[v] * abs(mx[v, j]), ew[v] + ex[v, j]) / sw for j in range(4)])
    return mean, absmean, n


def bound(n, absmean):
    """The derived bound on |computed - exact| of one coordinate: any-order float64 summation of n rounded products,
    divided by an any-order sum of n positive weights with one rounded division."""
    return Fraction(2 * int(n) + 4, 2 ** 53) * absmean


def image_candidates(scores, count, r0, r1):
    """Flat indices (row * K + slot) of ALL candidates of rows [r0, r1): slots [0, clamp(count[r], 0, K)) of every row."""
    K = scores.shape[1]
    c = np.clip(np.asarray(count, np.int64), 0, K)
    return np.concatenate([np.arange(r * K, r * K + c[r]) for r in range(r0, r1)] + [np.zeros(0, np.int64)]).astype(np.int64)
