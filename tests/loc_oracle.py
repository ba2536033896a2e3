"""float64 torch restatement of the location terms of mbx_loss_fwd_bwd_loc (include/mbx.h): l2, smooth_l1, giou, diou, ciou.
Every formula is written forward only; the gradients come from autograd, so nothing here shares a derivation with the
hand-written gradients of the kernel.  A min or max is a torch.where that takes its FIRST argument at a tie, max(0, x) one
that passes x only where x > 0, and atan2(w, h) is the constant 0 where w^2 + h^2 == 0: the conventions of the header, so
that the oracle is defined at the kinks too (torch.minimum / maximum would split the gradient there).  CIoU's trade-off
weight `a` is detached.  The confidence side is tests/focal_oracle.py's."""
import math

import numpy as np
import torch

from tests import focal_oracle as FO

TYPES = ("l2", "smooth_l1", "giou", "diou", "ciou")          # MBX_LOC_L2 = 0 .. MBX_LOC_CIOU = 4, in this order
EPS = 1e-7
BETA = 0.1                                                   # LOSS_LOC_BETA's default


def _min(a, b):
    return torch.where(a <= b, a, b)


def _max(a, b):
    return torch.where(a >= b, a, b)


def _relu(x):
    return torch.where(x > 0, x, torch.zeros_like(x))


def _atan2(w, h):
    flat = (w * w + h * h) == 0
    one = torch.ones_like(w)
    return torch.where(flat, torch.zeros_like(w), torch.atan2(torch.where(flat, one, w), torch.where(flat, one, h)))


def iou_parts(l, g):
    """The shared quantities of the IoU family for l, g [N, 4] (float64 tensors): a dict of [N] tensors."""
    x1, x2, y1, y2 = _min(l[:, 0], l[:, 2]), _max(l[:, 0], l[:, 2]), _min(l[:, 1], l[:, 3]), _max(l[:, 1], l[:, 3])
    gx1, gy1, gx2, gy2 = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    w, h, gw, gh = x2 - x1, y2 - y1, gx2 - gx1, gy2 - gy1
    iw = _relu(_min(x2, gx2) - _max(x1, gx1))
    ih = _relu(_min(y2, gy2) - _max(y1, gy1))
    inter = iw * ih
    union = w * h + gw * gh - inter
    cw = _max(x2, gx2) - _min(x1, gx1)
    ch = _max(y2, gy2) - _min(y1, gy1)
    rho2 = ((x1 + x2 - gx1 - gx2) ** 2 + (y1 + y2 - gy1 - gy2) ** 2) / 4
    return dict(w=w, h=h, gw=gw, gh=gh, inter=inter, union=union, iou=inter / (union + EPS), cw=cw, ch=ch, rho2=rho2)


def per_box(loc_type, l, g, beta=BETA):
    """L per pair for l, g [N, 4] float64 tensors -> [N]."""
    if loc_type == "l2":
        return 0.5 * ((l - g) ** 2).sum(1)
    if loc_type == "smooth_l1":
        d = (l - g).abs()
        return torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta).sum(1)
    q = iou_parts(l, g)
    if loc_type == "giou":
        c = q["cw"] * q["ch"]
        return 1 - q["iou"] + (c - q["union"]) / (c + EPS)
    diou = 1 - q["iou"] + q["rho2"] / (q["cw"] ** 2 + q["ch"] ** 2 + EPS)
    if loc_type == "diou":
        return diou
    assert loc_type == "ciou", loc_type
    v = (4 / math.pi ** 2) * (_atan2(q["gw"], q["gh"]) - _atan2(q["w"], q["h"])) ** 2
    a = (v / (1 - q["iou"] + v + EPS)).detach()
    return diou + a * v


def box_loss_and_grad(loc_type, l, g, beta=BETA):
    """(L [N], dL/dl [N, 4]) as float64 numpy for numpy boxes l, g [N, 4]; the inputs are widened, never rounded."""
    lt = torch.tensor(np.asarray(l, np.float64), requires_grad=True)
    L = per_box(loc_type, lt, torch.tensor(np.asarray(g, np.float64)), beta)
    grad, = torch.autograd.grad(L.sum(), lt)
    return L.detach().numpy(), grad.numpy()


def kink_distances(l, g, beta=BETA):
    """For boxes l, g [N, 4]: the distance of each pair to the nearest kink of any type, [N] float64 -- the coordinate ties
    of every min / max of the definition (the ordering of the prediction, the intersection, the enclosing box, the
    max(0, .) of the intersection sides) and |l_k - g_k| = beta."""
    l, g = np.asarray(l, np.float64), np.asarray(g, np.float64)
    lo = np.minimum(l[:, :2], l[:, 2:])
    hi = np.maximum(l[:, :2], l[:, 2:])
    side = np.minimum(hi, g[:, 2:]) - np.maximum(lo, g[:, :2])
    d = [np.abs(l[:, :2] - l[:, 2:]), np.abs(hi - g[:, 2:]), np.abs(lo - g[:, :2]), np.abs(side), np.abs(np.abs(l - g) - beta)]
    return np.concatenate(d, axis=1).min(1)


def make_loc_case(B, P, G):
    """tests.loss_cases.make_case(B, P, G) -- its match, z and x -- with boxes that mean something to an IoU: gt valid
    (xy ~ U(0, .6), wh ~ U(.05, .4)), dec ~ U(0, 1) and, for a positive, its gt box + N(0, .08) per coordinate in float32:
    most positives overlap their box, some are inverted (x1 > x2 or y1 > y2), some lie beside it.  Seeded by
    RandomState(77 P + B), drawn in the order xy, wh, dec, noise [B, P, 4]."""
    from tests.loss_cases import make_case
    c = make_case(B, P, G)
    rng = np.random.RandomState(77 * P + B)
    xy, wh = rng.uniform(0, .6, (B, G, 2)), rng.uniform(.05, .4, (B, G, 2))
    c["gt"] = np.concatenate([xy, xy + wh], axis=2).astype(np.float32)
    c["dec"] = rng.uniform(0, 1, (B, P, 4)).astype(np.float32)
    noise = rng.normal(0, .08, (B, P, 4)).astype(np.float32)
    b, p = np.nonzero(c["match"] >= 0)
    c["dec"][b, p] = c["gt"][b, c["match"][b, p]] + noise[b, p]
    return c


def positives(c):
    """(l, g) [n_pos, 4] float64 of case c, in row-major order of the positives."""
    b, p = np.nonzero(c["match"] >= 0)
    return c["dec"][b, p].astype(np.float64), c["gt"][b, c["match"][b, p]].astype(np.float64)


def census(l, g):
    """(inverted, disjoint, overlapping) counts of pairs l, g [N, 4]: a prediction with x1 > x2 or y1 > y2; a pair whose
    intersection is empty once the prediction is put in order; a pair whose intersection has an area."""
    lo, hi = np.minimum(l[:, :2], l[:, 2:]), np.maximum(l[:, :2], l[:, 2:])
    side = np.minimum(hi, g[:, 2:]) - np.maximum(lo, g[:, :2])
    inverted = (l[:, 0] > l[:, 2]) | (l[:, 1] > l[:, 3])
    disjoint = (side <= 0).any(1)
    return int(inverted.sum()), int(disjoint.sum()), int((~disjoint).sum())


def loc_loss(loc_type, decoded, conf_in, conf_is_logit, gt, match, alpha, beta=BETA, gamma=0.0, w_pos=1.0, w_neg=1.0,
             neg_per_pos=0, min_neg=0):
    """dict(loc_loss float64, dl [B,P,4] float64, L [n_pos] float64 in row-major order of the positives, plus the
    confidence side of tests/focal_oracle.focal_loss: mask, n_neg, conf_loss, d_conf_in) for grad_scale = 1.  `beta` is
    rounded to float32 first, as the C ABI receives it."""
    beta = float(np.float32(beta))
    decoded, gt, match = np.asarray(decoded, np.float32), np.asarray(gt, np.float32), np.asarray(match)
    out = FO.focal_loss(decoded, conf_in, conf_is_logit, gt, match, alpha, gamma, w_pos, w_neg, neg_per_pos, min_neg)
    b, p = np.nonzero(match >= 0)
    dl = np.zeros(decoded.shape, np.float64)
    L = np.zeros((0,), np.float64)
    if b.size:
        L, grad = box_loss_and_grad(loc_type, decoded[b, p], gt[b, match[b, p]], beta)
        dl[b, p] = float(alpha) * grad
    return dict(mask=out["mask"], n_neg=out["n_neg"], conf_loss=out["conf_loss"], d_conf_in=out["d_conf_in"],
                loc_loss=float(alpha) * float(L.sum()), dl=dl, L=L)
