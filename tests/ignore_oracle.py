"""numpy restatements of the ignore band (include/mbx.h): mbx_match_ignore as a plain loop on tests/extend_oracle.iou_row, and
mbx_loss_fwd_bwd_ignore by COMPACTION -- the ignored priors of an image are dropped, tests/quality_oracle.quality_loss (or
tests/loc_oracle.loc_loss without a quality target) runs on what is left, and the results are scattered back with zeros.
Removing priors keeps the relative index order of the others, so mining's tie-break stands."""
import numpy as np

from tests import extend_oracle as EO
from tests import loc_oracle as LO
from tests import quality_oracle as QO

FREE, IGNORED = -1, -2                                       # MBX_MATCH_FREE, MBX_MATCH_IGNORED


def ignore(boxes, per_image, gt, n_gt, status, match, thr):
    """(match int32 [B,P] with the band written in, n_ignored int32 [B]).  boxes [P,4], or [B,P,4] when per_image.  thr is
    the float32 the C ABI is given, widened; `>=`, not strict; a NaN IoU passes nothing."""
    boxes, gt = np.asarray(boxes, np.float32), np.asarray(gt, np.float32)
    thr = float(np.float32(thr))
    out = np.array(match, np.int32, copy=True)
    B, P = out.shape
    G = gt.shape[1]
    n_ignored = np.zeros(B, np.int32)
    for b in range(B):
        n = int(n_gt[b])
        if int(status[b]) != 0 or n <= 0 or n > G:
            continue
        own = boxes[b] if per_image else boxes
        for p in range(P):
            if out[b, p] != FREE:
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                iou = EO.iou_row(own[p], gt[b, :n])
                hit = bool((iou >= thr).any())
            if hit:
                out[b, p] = IGNORED
                n_ignored[b] += 1
    return out, n_ignored


def best_iou(boxes, gt, n_gt):
    """[B,P] float64: the largest IoU of prior p with the boxes of image b (0 where the image has none)."""
    boxes, gt = np.asarray(boxes, np.float32), np.asarray(gt, np.float32)
    B, P = gt.shape[0], boxes.shape[0]
    out = np.zeros((B, P))
    for b in range(B):
        if n_gt[b] > 0:
            out[b] = [EO.iou_row(boxes[p], gt[b, :n_gt[b]]).max() for p in range(P)]
    return out


def loss(mode, loc_type, decoded, conf_in, conf_is_logit, gt, match, alpha, gamma, w_pos=1.0, w_neg=1.0, neg_per_pos=0,
         min_neg=0, beta=LO.BETA):
    """dict(kept bool [B,P], n_neg [B], loc_loss, conf_loss float64, dl [B,P,4], d_conf_in [B,P] float64, q_stats [B,2]) for
    grad_scale = 1.  mode: "qfl", "varifocal" or None (no quality target: the focal confidence term)."""
    decoded, gt, match = np.asarray(decoded, np.float32), np.asarray(gt, np.float32), np.asarray(match)
    conf_in = np.asarray(conf_in, np.float32)
    B, P = match.shape
    kept = match != IGNORED
    out = dict(kept=kept, n_neg=np.zeros(B, np.int64), loc_loss=0.0, conf_loss=0.0, dl=np.zeros((B, P, 4)),
               d_conf_in=np.zeros((B, P)), q_stats=np.zeros((B, 2)))
    for b in range(B):
        k = np.nonzero(kept[b])[0]
        if not k.size:
            continue
        sub = (decoded[b:b + 1, k], conf_in[b:b + 1, k], conf_is_logit, gt[b:b + 1], match[b:b + 1, k], alpha)
        if mode is None:
            r = LO.loc_loss(loc_type, *sub, beta, gamma, w_pos, w_neg, neg_per_pos, min_neg)
        else:
            r = QO.quality_loss(mode, loc_type, *sub, gamma, w_pos, w_neg, neg_per_pos, min_neg, beta)
            out["q_stats"][b] = r["q_stats"][0]
        out["n_neg"][b] = r["n_neg"][0]
        out["loc_loss"] += r["loc_loss"]
        out["conf_loss"] += r["conf_loss"]
        out["dl"][b, k] = r["dl"][0]
        out["d_conf_in"][b, k] = r["d_conf_in"][0]
    return out
