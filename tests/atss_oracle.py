"""numpy float64 restatement of mbx_match_atss (include/mbx.h): ATSS matching behind the bipartite match.  Plain loops per
image, box and prior; every float64 operation is the header's, in its order, so `match`, `n_extra` and `thr` are compared
bit for bit with the kernel's."""
import numpy as np

from tests.extend_oracle import iou_row


def centres(boxes):
    """(cx, cy) float64 of corner boxes [n,4] given as float32: (x1 + x2) * 0.5, (y1 + y2) * 0.5."""
    b = np.asarray(boxes, np.float32).astype(np.float64).reshape(-1, 4)
    return (b[:, 0] + b[:, 2]) * 0.5, (b[:, 1] + b[:, 3]) * 0.5


def distances(priors, box):
    """d2 float64 [P] of every prior's centre to the box's: dx * dx + dy * dy."""
    cx, cy = centres(priors)
    bx, by = centres(box)
    dx, dy = cx - bx[0], cy - by[0]
    with np.errstate(invalid="ignore", over="ignore"):
        return dx * dx + dy * dy


def candidates(priors, level_start, box, topk):
    """The candidate priors of one box in ascending index: per level the min(topk, size) smallest d2, equal d2 to the lowest
    index, a NaN behind every number."""
    d2 = distances(priors, box)
    nan = np.isnan(d2)
    d2 = np.where(nan, 0.0, d2)
    out = []
    for lo, hi in zip(level_start[:-1], level_start[1:]):
        order = lo + np.lexsort((np.arange(lo, hi), d2[lo:hi], nan[lo:hi]))       # by (is NaN, d2, index)
        out += sorted(int(p) for p in order[:min(int(topk), hi - lo)])
    return out


def threshold(ious):
    """mean + sample standard deviation of the candidate IoUs, serial sums from 0.0 in the order given."""
    m = len(ious)
    s = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in ious:
            s = s + v
        mean = s / np.float64(m)
        q = np.float64(0.0)
        for v in ious:
            d = v - mean
            q = q + d * d
        std = np.sqrt(q / np.float64(m - 1)) if m > 1 else np.float64(0.0)
        return mean + std


def positives(priors, level_start, box, topk):
    """(candidates [m], their IoUs [m], thr, positive mask [m]) of one box."""
    priors = np.asarray(priors, np.float32)
    cand = candidates(priors, level_start, box, topk)
    ious = np.array([iou_row(priors[p], box)[0] for p in cand], np.float64)
    thr = threshold(ious)
    g = np.asarray(box, np.float32).astype(np.float64).reshape(4)
    cx, cy = centres(priors[cand])
    inside = (g[0] < cx) & (cx < g[2]) & (g[1] < cy) & (cy < g[3])
    with np.errstate(invalid="ignore"):
        pos = (ious > 0) & (ious >= thr) & inside
    return cand, ious, thr, pos


def atss(priors, level_start, gt, n_gt, status, match, topk):
    """(match int32 [B,P], n_extra int32 [B], thr float64 [B,G])."""
    priors, gt = np.asarray(priors, np.float32), np.asarray(gt, np.float32)
    level_start = [int(v) for v in level_start]
    out = np.array(match, np.int32, copy=True)
    B, P = out.shape
    G = gt.shape[1]
    assert level_start[0] == 0 and level_start[-1] == P and all(a < b for a, b in zip(level_start, level_start[1:]))
    n_extra = np.zeros(B, np.int32)
    thr = np.zeros((B, G), np.float64)
    for b in range(B):
        n = int(n_gt[b])
        if int(status[b]) != 0 or n <= 0 or n > G:
            continue
        best_iou, best_j = {}, {}
        for j in range(n):
            cand, ious, thr[b, j], pos = positives(priors, level_start, gt[b, j], topk)
            for p, v, is_pos in zip(cand, ious, pos):
                if is_pos and out[b, p] < 0 and (p not in best_iou or v > best_iou[p]):     # strictly larger: lowest j stays
                    best_iou[p], best_j[p] = v, j
        for p, j in best_j.items():
            out[b, p] = j
        n_extra[b] = len(best_j)
    return out, n_extra, thr
