"""numpy float64 restatement of mbx_match_extend (include/mbx.h): threshold matching behind the bipartite match.  A plain
loop per image and per prior; every float64 operation is the header's, in its order, so the decisions are compared bit
for bit with the kernel's."""
import numpy as np


def iou_row(prior, boxes):
    """IoU of one prior with each of `boxes` [n,4] (corners), float64 on the float32 values, the prior first:
    iw = min(x2) - max(x1), ih likewise; inter = iw > 0 and ih > 0 ? iw * ih : 0; uni = area_p + area_j - inter;
    iou = uni > 0 ? inter / uni : 0."""
    p = np.asarray(prior, np.float32).astype(np.float64)
    g = np.asarray(boxes, np.float32).astype(np.float64).reshape(-1, 4)
    area_p = (p[2] - p[0]) * (p[3] - p[1])
    area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    iw = np.minimum(p[2], g[:, 2]) - np.maximum(p[0], g[:, 0])
    ih = np.minimum(p[3], g[:, 3]) - np.maximum(p[1], g[:, 1])
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
    uni = area_p + area_g - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 0.0)


def extend(priors, gt, n_gt, status, match, iou_threshold):
    """(extended match int32 [B,P], n_extra int32 [B]).  iou_threshold is the float32 the C ABI is given, widened."""
    priors, gt = np.asarray(priors, np.float32), np.asarray(gt, np.float32)
    thr = float(np.float32(iou_threshold))
    out = np.array(match, np.int32, copy=True)
    B, P = out.shape
    n_extra = np.zeros(B, np.int32)
    for b in range(B):
        n = int(n_gt[b])
        if int(status[b]) != 0 or n <= 0:
            continue
        for p in range(P):
            if out[b, p] >= 0:
                continue
            iou = iou_row(priors[p], gt[b, :n])
            j = int(np.argmax(iou))                            # the first of equal maxima: the lowest index
            if iou[j] > thr:
                out[b, p] = j
                n_extra[b] += 1
    return out, n_extra
