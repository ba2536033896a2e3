"""The oracle of the weighted-boxes-fusion tests (mbx_merge_detections_wbf): the definition of include/mbx.h restated in
numpy, one vectorised IoU per candidate -- never built from the code under test.  The IoU is oracle.ref_numpy.nms_greedy's,
term by term, with the areas handed in (tests/test_wbf_cpu.py ties the two); every other operation is one rounded float64
operation in the order the header gives, so every output is exact."""
import numpy as np

from oracle import ref_numpy as R  # noqa: F401  (the IoU restated below)
from tests.merge_oracle import CAND_LIMIT
from tests.soft_oracle import image_candidates, is_live  # noqa: F401  (the candidate set and the live rule are the same)

AVG, MAX = 1, 2


def iou_fused(F, A, x, a):
    """IoU of every fused box F [n,4] (areas A [n]) with the candidate x [4] (area a), float64, in R.nms_greedy's operation
    order with the fused box as the EARLIER box."""
    iw = np.minimum(F[:, 2], x[2]) - np.maximum(F[:, 0], x[0])
    ih = np.minimum(F[:, 3], x[3]) - np.maximum(F[:, 1], x[1])
    inter = np.where((iw > 0.0) & (ih > 0.0), iw * ih, 0.0)
    union = A + a - inter
    pos = union > 0.0
    return np.where(pos, inter / np.where(pos, union, 1.0), 0.0)


def wbf(cand_boxes, cand_scores, conf_type, thr, min_score, views):
    """Fusion of one image's candidates, given in ascending flat-index order.  Returns the clusters in OUTPUT order (before
    the max_det cut): (F [n,4] f64, score [n] f32, first [n]: position of the founder in the candidates' order, members [n])."""
    b = np.asarray(cand_boxes, np.float64).reshape(-1, 4)
    s = np.asarray(cand_scores, np.float32).reshape(-1)
    t = s.astype(np.float64)
    live = np.flatnonzero(is_live(t, min_score))                          # finite and positive: -t orders them like the device's keys
    order = live[np.argsort(-t[live], kind="stable")]
    n_max = len(order)
    F, A, S, X = np.zeros((n_max, 4)), np.zeros(n_max), np.zeros(n_max), np.zeros((n_max, 4))
    n, first, nc = np.zeros(n_max, np.int64), np.zeros(n_max, np.int64), 0
    for c in order:
        x, tc = b[c], t[c]
        a = (x[2] - x[0]) * (x[3] - x[1])
        m = -1
        if nc:
            o = iou_fused(F[:nc], A[:nc], x, a)
            m = int(np.argmax(o))                                         # the first of equal maxima: the lowest cluster number
            if not o[m] > np.float64(thr):
                m = -1
        if m >= 0:
            S[m] = S[m] + tc
            X[m] = X[m] + tc * x
            n[m] += 1
            F[m] = X[m] / S[m]
            A[m] = (F[m, 2] - F[m, 0]) * (F[m, 3] - F[m, 1])
        else:
            S[nc], X[nc], n[nc], F[nc], A[nc], first[nc] = tc, tc * x, 1, x, a, c
            nc += 1
    q = S[:nc] / n[:nc].astype(np.float64) if conf_type == AVG else t[first[:nc]]
    assert conf_type in (AVG, MAX)
    if views > 1:
        q = (q * np.minimum(n[:nc], views).astype(np.float64)) / np.float64(views)
    score = q.astype(np.float32)
    out = np.argsort(-score, kind="stable")                               # >= 0 and finite: the order of the device's keys
    return F[:nc][out], score[out], first[:nc][out], n[:nc][out]


def wbf_oracle(boxes, scores, count, image_rows, conf_type, thr, min_score, views, cand_limit=CAND_LIMIT):
    """Per image: (F, score, first as FLAT index, members, status) of all its clusters in output order.  An image above the
    candidate limit has status 1 and no clusters."""
    fb, fs = np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(scores, np.float32).reshape(-1)
    out = []
    for i in range(len(image_rows) - 1):
        flat = image_candidates(scores, count, int(image_rows[i]), int(image_rows[i + 1]))
        if len(flat) > cand_limit:
            out.append((np.zeros((0, 4)), np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64), 1))
            continue
        F, sc, first, n = wbf(fb[flat], fs[flat], conf_type, thr, min_score, views)
        out.append((F, sc, flat[first], n, 0))
    return out


def expected_arrays(result, max_det):
    """The kernel's six outputs for wbf_oracle's result, cut to max_det: unused slots 0 / 0 / -1 / 0."""
    k = len(result)
    ob, osc = np.zeros((k, max_det, 4), np.float64), np.zeros((k, max_det), np.float32)
    src, votes = np.full((k, max_det), -1, np.int32), np.zeros((k, max_det), np.int32)
    cnt, st = np.zeros((k,), np.int32), np.zeros((k,), np.int32)
    for i, (F, sc, first, n, status) in enumerate(result):
        m = min(len(sc), max_det)
        ob[i, :m], osc[i, :m], src[i, :m], votes[i, :m], cnt[i], st[i] = F[:m], sc[:m], first[:m], n[:m], m, status
    return ob, osc, src, cnt, st, votes
