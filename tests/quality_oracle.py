"""numpy restatement of mbx_loss_fwd_bwd_quality (include/mbx.h): the IoU of a positive's prediction with its box as its
confidence target, by the Quality Focal Loss ("qfl") or the Varifocal Loss ("varifocal").  s, c, w come from
tests/focal_oracle.scw (float32, as the kernel takes them), the negatives and the selection from
tests/focal_oracle.focal_loss, the location side from tests/loc_oracle.loc_loss, q from tests/loc_oracle.iou_parts; the
positive term and its derivative are the closed form of the header, in float64 from the widened float32 values."""
import numpy as np
import torch

from tests import focal_oracle as FO
from tests import loc_oracle as LO

MODES = ("qfl", "varifocal")                                 # MBX_QUALITY_QFL = 1, MBX_QUALITY_VFL = 2
QUALITY = {"none": 0, "qfl": 1, "varifocal": 2}


def iou(l, g):
    """q [N] float64 for boxes l, g [N, 4]: the inputs are widened, never rounded."""
    l, g = np.asarray(l, np.float64).reshape(-1, 4), np.asarray(g, np.float64).reshape(-1, 4)
    return LO.iou_parts(torch.tensor(l), torch.tensor(g))["iou"].numpy()


def positive_terms(mode, q, s, c, w, gamma, w_pos=1.0):
    """(L, dL/ds) [N] float64 of positives with targets q and float64 (widened) s, c, w: L = -w_pos M t,
    t = q log c + (1 - q) log w.  qfl: M = |q - s|^gamma, dM/ds = -gamma |q - s|^(gamma-1) sgn(q - s), exactly 0 at q == s,
    and with gamma == 0 M is 1 and the dM term is left out; varifocal: M = q."""
    assert mode in MODES, mode
    q, s, c, w = (np.asarray(a, np.float64) for a in (q, s, c, w))
    t = q * np.log(c) + (1.0 - q) * np.log(w)
    dt = q / c - (1.0 - q) / w
    if mode == "varifocal" or gamma == 0:
        M = q if mode == "varifocal" else np.ones_like(q)
        return -w_pos * M * t, -w_pos * (M * dt)
    d = q - s
    a = np.abs(d)
    M = a ** gamma
    with np.errstate(divide="ignore", invalid="ignore"):
        dM = np.where(d == 0, 0.0, -gamma * a ** (gamma - 1.0) * np.sign(d))
    return -w_pos * M * t, -w_pos * (dM * t + M * dt)


def quality_loss(mode, loc_type, decoded, conf_in, conf_is_logit, gt, match, alpha, gamma, w_pos=1.0, w_neg=1.0, neg_per_pos=0,
                 min_neg=0, beta=LO.BETA):
    """dict(mask, n_neg, loc_loss, dl, conf_loss float64, d_conf_in [B,P] float64, q, L [n_pos] in row-major order of the
    positives, q_stats [B,2] float64, neg_loss) for grad_scale = 1.  The weights and gamma are rounded to float32 first, as
    the C ABI receives them."""
    gamma, w_pos, w_neg = (float(np.float32(v)) for v in (gamma, w_pos, w_neg))
    decoded, gt, match = np.asarray(decoded, np.float32), np.asarray(gt, np.float32), np.asarray(match)
    conf_in = np.asarray(conf_in, np.float32)
    B, P = match.shape
    # the location side, the selection and the negatives' gradients: the focal oracle's, its positives weighed 0
    base = LO.loc_loss(loc_type, decoded, conf_in, conf_is_logit, gt, match, alpha, beta, gamma, 0.0, w_neg, neg_per_pos, min_neg)
    pos, mask = match >= 0, base["mask"]
    s, c, w = FO.scw(conf_in, conf_is_logit)
    s64, c64, w64 = (a.astype(np.float64) for a in (s, c, w))
    ds = s64 * (1.0 - s64) if conf_is_logit else np.ones((B, P))
    with np.errstate(divide="ignore", invalid="ignore"):
        lc, lw = np.log(c).astype(np.float64), np.log(w).astype(np.float64)     # the float32 logarithms of focal_loss
    neg_term, _ = FO.terms(c64, w64, ds, np.zeros_like(pos), mask, gamma, 0.0, w_neg, lc, lw)
    neg_loss = float(sum(float(np.sum(neg_term[b, ~pos[b]])) for b in range(B)))
    d_in = np.where(pos, 0.0, base["d_conf_in"].astype(np.float64))
    b, p = np.nonzero(pos)
    q = np.zeros((0,), np.float64)
    L = np.zeros((0,), np.float64)
    q_stats = np.zeros((B, 2), np.float64)
    if b.size:
        q = iou(decoded[b, p], gt[b, match[b, p]])
        L, dLds = positive_terms(mode, q, s64[b, p], c64[b, p], w64[b, p], gamma, w_pos)
        d_in[b, p] = dLds * ds[b, p]
        for i in range(B):
            q_stats[i] = float(np.sum(q[b == i])), float(np.sum(b == i))
    return dict(mask=mask, n_neg=base["n_neg"], loc_loss=base["loc_loss"], dl=base["dl"], conf_loss=neg_loss + float(L.sum()),
                d_conf_in=d_in, q=q, L=L, q_stats=q_stats, neg_loss=neg_loss, s=s64[b, p] if b.size else q)
