"""numpy restatement of mbx_loss_fwd_bwd_focal (include/mbx.h): the focal loss on the confidence term, with or without
hard-negative mining.  s, c, w and the two logarithms are taken in float32 exactly as oracle.ref_numpy takes them (its
np.log is applied to the float32 c and w, then widened); everything after them -- the powers, the products, the sums -- is
float64, in ref_numpy's order, so that gamma = 0 with unit weights IS ref_numpy.add_loss / add_loss_grads, bit for bit.
The selection under mining is tests/mined_oracle.select: integer work on float bits, exact."""
import numpy as np

from oracle import ref_numpy as R
from tests import mined_oracle as MO


def scw(conf_in, conf_is_logit):
    """(s, c, w) in float32: s = sigmoid(conf_in) or conf_in, c = s + 1e-10, w = (1 - c) + 1e-10 (ref_numpy.add_loss)."""
    conf_in = np.asarray(conf_in, np.float32)
    with np.errstate(over="ignore"):
        s = R.sigmoid_f32(conf_in) if conf_is_logit else conf_in
    c = (s + np.float32(R.SMALL_EPSILON)).astype(np.float32)
    w = ((np.float32(1.0) - c) + np.float32(R.SMALL_EPSILON)).astype(np.float32)
    return s, c, w


def terms(c, w, ds, pos, counted, gamma, w_pos, w_neg, lc=None, lw=None):
    """(term, d term / d conf_in) per prior in the dtype of c and w: positives where `pos`, negatives where `counted`, 0
    elsewhere; ds = ds/d conf_in.  With gamma == 0 the power is 1 and the gamma * x^(gamma-1) * log term is left out.  The
    products are taken in the order that makes gamma = 0 with unit weights ref_numpy's own expressions, -ds / c and ds / w.
    lc, lw: log c and log w where the caller has taken them already (default: np.log in the dtype of c and w)."""
    dt = c.dtype.type
    gamma, w_pos, w_neg = dt(gamma), dt(w_pos), dt(w_neg)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        lc, lw = np.log(c) if lc is None else lc, np.log(w) if lw is None else lw
        if gamma == 0:
            wg, cg = np.ones_like(w), np.ones_like(c)
            g_pos, g_neg = -(ds * wg) / c, (ds * cg) / w
        else:
            wg, cg = np.power(w, gamma), np.power(c, gamma)
            g_pos = gamma * (wg / w) * lc * ds - (ds * wg) / c
            g_neg = (ds * cg) / w - gamma * (cg / c) * lw * ds
        zero = np.zeros_like(c)
        term = np.where(pos, -(w_pos * (wg * lc)), np.where(counted, -(w_neg * (cg * lw)), zero))
        grad = np.where(pos, w_pos * g_pos, np.where(counted, w_neg * g_neg, zero))
    return term, grad


def focal_loss(decoded, conf_in, conf_is_logit, gt, match, alpha, gamma, w_pos, w_neg, neg_per_pos, min_neg):
    """dict(mask, n_neg, loc_loss, conf_loss, d_locs, d_conf_in) for grad_scale = 1.  `decoded` are prior-decoded
    locations, as the C ABI takes them; `mask` marks the negatives that count (every one when neg_per_pos == 0)."""
    decoded, conf_in = np.asarray(decoded, np.float32), np.asarray(conf_in, np.float32)
    match = np.asarray(match)
    B, P = match.shape
    pos = match >= 0
    if neg_per_pos:
        mask, K = MO.select(conf_in, match, neg_per_pos, min_neg)
    else:
        assert min_neg == 0
        mask, K = ~pos, (P - pos.sum(1)).astype(np.int32)
    s, c, w = scw(conf_in, conf_is_logit)
    s64 = s.astype(np.float64)
    ds = s64 * (1.0 - s64) if conf_is_logit else np.ones((B, P))
    with np.errstate(divide="ignore", invalid="ignore"):
        lc, lw = np.log(c).astype(np.float64), np.log(w).astype(np.float64)
    term, grad = terms(c.astype(np.float64), w.astype(np.float64), ds, pos, mask, gamma, w_pos, w_neg, lc, lw)
    conf = 0.0
    for b in range(B):                                        # ref_numpy.add_loss's order: the positives, then the negatives
        if pos[b].any():
            conf += float(np.sum(term[b, pos[b]]))
        conf += float(np.sum(term[b, ~pos[b]]))               # an unselected negative's term is 0
    conf_loss = np.float32(conf)
    d_in = grad.astype(np.float32)
    # the location side is ref_numpy's own (the confidences it is given play no part in it)
    zero_priors = np.zeros((P, 4), np.float32)
    n = pos.sum(1).astype(np.int32)
    loc_loss = R.add_loss(decoded, np.full((B, P), 0.5, np.float32), gt, n, zero_priors, alpha, match=match)["loc_loss"]
    d_locs, _ = R.add_loss_grads(decoded, np.zeros((B, P), np.float32), gt, zero_priors, alpha, match)
    return dict(mask=mask, n_neg=K, loc_loss=loc_loss, conf_loss=conf_loss, d_locs=d_locs, d_conf_in=d_in)
